"""The per-lane k-d walk's control (no GPU): the step at a branch is kd_descend, the pops are kd_resume_closest /
kd_resume_occluded / kd_resume_tagged (nt_composite.hpp), and the per-lane walkers -- fixed N and run-time n -- call them
instead of carrying the text, except the ones a measurement kept on their own copy, which EXCEPTIONS lists with the figures.
Read off the sources, so a copy that grows back fails here before it can drift from the rest.
The wave-uniform walks (composite_packet, xray_packet) are another algorithm and keep their own step; composite_persistent keeps
its copy inside its state machine."""
import re

import support as sup

FILES = ("nt_composite.hpp", "nt_var.hip", "nt_xray.hpp")
# (file, head of the function): the per-lane walkers; for xray_var the kernel's body
WALKERS = (
    ("nt_composite.hpp", "__noinline__ bool trace_closest("),
    ("nt_composite.hpp", "NT_OCCL_ATTR bool trace_occluded("),
    ("nt_composite.hpp", "__noinline__ bool trace_closest_t("),
    ("nt_composite.hpp", "__noinline__ bool trace_occluded_t("),
    ("nt_var.hip", "__noinline__ bool trace_closest_var("),
    ("nt_var.hip", "__noinline__ bool trace_occluded_var("),
    ("nt_var.hip", "__noinline__ bool trace_closest_var_t("),
    ("nt_var.hip", "__noinline__ bool trace_occluded_var_t("),
    ("nt_var.hip", "void xray_var("),
)
# Walkers kept on their own copy of the text, each with what kept it off the helpers (profiles/kd_walk_ab.jsonl: parent and head
# libraries alternated on one MI355X, five runs each, the head's median against the parent's min..max;
# profiles/kd_walk_codeobjects.txt: the kernels' registers).  With their own text their code is the parent's again,
# instruction for instruction (in the units that trace_closest_t changes it sits at other addresses).
EXCEPTIONS = (
    # tools/lens_time.py, cell120_n4 lit: plain 29.34 ms against 28.65..28.85, pinhole 29.42 against 28.46..28.55;
    # tools/query_time.py: query 7.99 ms against 7.83..7.86, normals 7.98 against 7.82..7.85, boxed 6.05 against 5.91..5.94
    ("nt_composite.hpp", "__noinline__ bool trace_closest("),
    ("nt_composite.hpp", "NT_OCCL_ATTR bool trace_occluded("),
    # query_occluded_t<3>, <8>, <9>, <10> save 16 SGPRs around its call (spill count 0 -> 16) in every helper form tried
    ("nt_composite.hpp", "__noinline__ bool trace_occluded_t("),
    # tools/xray_time.py, feature16_n16 counts (xray_var<true>): 9.80 ms against 9.62..9.68
    ("nt_var.hip", "void xray_var("),
)
DESCENT = ("nt_composite.hpp", "KdStep kd_descend(")
HELPERS = (DESCENT,) + tuple(("nt_composite.hpp", h) for h in (
    "float branch_t(", "float kd_t_far_below(", "bool kd_resume_closest(", "bool kd_resume_occluded(", "float kd_t_far_below_tagged(",
    "bool kd_resume_tagged("))
PERSISTENT = ("nt_composite.hpp", "void composite_persistent(")
WAVE_UNIFORM = (("nt_composite.hpp", "void composite_packet("), ("nt_xray.hpp", "void xray_packet("))
SPLIT_TEST = r"t < 0\.0f \|\| t > t_far"


def _body(where):
    return sup.function_body(sup.source(where[0]), where[1])


def _without(text, bodies):
    for b in bodies:
        assert text.count(b) == 1
        text = text.replace(b, "")
    return text


def test_the_descent_rule_exists_once():
    allowed = [_body(w) for w in (DESCENT, PERSISTENT) + WAVE_UNIFORM + EXCEPTIONS]
    for b in allowed:
        assert len(re.findall(SPLIT_TEST, b)) == 1
    text = "".join(sup.source(f) for f in FILES)
    assert len(re.findall(SPLIT_TEST, text)) == len(allowed) == 4 + len(EXCEPTIONS)
    assert not re.findall(SPLIT_TEST, _without(text, allowed))


def test_every_per_lane_walker_calls_the_helpers():
    assert len(WALKERS) == 9 and len(set(WALKERS)) == 9
    for w in WALKERS:
        if w in EXCEPTIONS:
            continue
        body = _body(w)
        assert len(re.findall(r"\bkd_descend\(", body)) == 1, w
        assert len(re.findall(r"\bkd_resume_(closest|occluded|tagged)\(", body)) == 1, w
        assert "w.stack[" not in body and "w.ray[" not in body, w
    # which pop each flavour takes, and where t_far of the resumed frame comes from: the plain stack's reload follows the pop in
    # the walker, the tagged stack's scan sits in kd_resume_tagged
    for w, pop in zip(WALKERS, ("closest", "occluded", "tagged", "occluded", "closest", "occluded", "tagged", "occluded", "closest")):
        if w in EXCEPTIONS:
            continue
        assert "kd_resume_%s(" % pop in _body(w), w
        assert len(re.findall(r"\bkd_t_far_below\(", _body(w))) == (0 if pop == "tagged" else 1), w
    assert len(re.findall(r"\bkd_t_far_below_tagged\(", _body(("nt_composite.hpp", "bool kd_resume_tagged(")))) == 1
    # the occlusion walks keep the reference's far-child rule between the step and the far child (tracer.hpp:1298)
    for w in WALKERS:
        assert bool(re.search(r"if \((s\.)?t < ldistance\) \{ node = -1; break; \}", _body(w))) == ("occluded" in w[1]), w


def test_branch_t_is_called_by_the_helpers_alone():
    text = "".join(sup.source(f) for f in FILES)
    rest = _without(text, [_body(w) for w in HELPERS + (PERSISTENT,) + EXCEPTIONS])
    assert "branch_t(" not in rest
    # and the plain and the tagged reload of a resumed frame's t_far are defined once each
    for name in ("kd_t_far_below", "kd_t_far_below_tagged"):
        assert len(re.findall(r"float %s\(" % name, text)) == 1
