"""What the whole-view settings -- clip planes, depth cues, outlines, ambient occlusion, BoxScene's face lines -- refuse of a
render, and what the entry points that return their buffers (and the adaptive mask's) refuse before they touch a device: every
answer byte for byte against tests/view_setting_refusals.py, which was written down from the library before the five check
functions became one table.  No GPU: a refusal that reached a device would show as another error here."""
import ctypes as C
import os

import numpy as np
import pytest

import fixtures as fx
import ntracer_amd
import ray_query_cases as rq
import view_setting_refusals as vr
import support as sup
from ntracer_amd import _lib, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 8, 4

# how a scene gets each setting, and loses it
ON = {
    "clip": lambda s: s.set_clip_planes([((1.0,) + (0.0,) * (s.dimension - 1), 1.0)]),
    "cue": lambda s: s.set_depth_cue(1.0, 2.0),
    "outlines": lambda s: s.set_outlines(),
    "ao": lambda s: s.set_ambient_occlusion(4, 1.0),
    "face lines": lambda s: s.set_face_lines(),
    "adaptive": lambda s: s.set_adaptive_supersampling(0.1),
}
OFF = {
    "clip": lambda s: s.set_clip_planes(None),
    "cue": lambda s: s.set_depth_cue(None),
    "outlines": lambda s: s.set_outlines(None),
    "ao": lambda s: s.set_ambient_occlusion(None),
    "face lines": lambda s: s.set_face_lines(None),
    "adaptive": lambda s: s.set_adaptive_supersampling(None),
}
COMPOSITE = ("clip", "cue", "outlines", "ao")          # in the order of precedence


# cause -> (what sets it up on the scene, what takes it away again, the options of the call)
CAUSES = {
    "supersampling": (lambda s: s.set_supersampling(2), lambda s: s.set_supersampling(1), None),
    "bands": (None, None, dict(band_world=2)),
    "collect_stats": (None, None, dict(collect_stats=1)),
    "lens": (lambda s: s.set_lens(tracern.Lens.pinhole(W, H, 0.8)), lambda s: s.set_lens(None), None),
    "parallel": (lambda s: s.set_parallel_projection(2.0), lambda s: s.set_parallel_projection(None), None),
    "ao": (ON["ao"], OFF["ao"], None),
    "outlines": (ON["outlines"], OFF["outlines"], None),
    "cue": (ON["cue"], OFF["cue"], None),
}


def _scene_for(setting, cause=None):
    if setting == "face lines":
        return tracern.BoxScene(5)
    g, n, flat = rq.scene("feature5_n5" if cause == "solids" else "cell120_n4")
    return tracern.CompositeScene.from_flat(n, flat)


class _Renders:
    """nt_render, nt_render_device and nt_render_frames_device of one scene into one marked destination"""

    def __init__(self, scene):
        self.scene, n = scene, scene.dimension
        self.fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in fx.RGBX8])
        self.fst = self.fmt._as_struct()
        self.size = self.fmt.pitch * H
        self.dest = (C.c_char * self.size)(*([0x4E] * self.size))
        self.origins, self.axes = np.zeros((1, n), np.float32), np.eye(n, dtype=np.float32)[None].copy()

    def answers(self, fields):
        """[(status, message)] of the three forms"""
        L, h = _lib.lib(), self.scene._handle
        opts = None if fields is None else sup.render_opts(**fields)
        po = None if opts is None else C.byref(opts)
        out = []
        for call in (lambda: L.nt_render(h, self.dest, self.size, C.byref(self.fst), po, None),
                     lambda: L.nt_render_device(h, self.dest, self.size, C.byref(self.fst), po, None),
                     lambda: L.nt_render_frames_device(h, self.dest, self.size, 1, self.origins.ctypes.data_as(_lib.f32p),
                                                       self.axes.ctypes.data_as(_lib.f32p), C.byref(self.fst), po, None)):
            status = call()
            out.append((status, _lib.last_error()))
        return out

    def untouched(self):
        return bytes(self.dest) == b"\x4e" * self.size


def render_answers(setting, cause):
    """the three render forms' answers with `setting` on and `cause` in the way, and whether the destination is as it was"""
    scene = _scene_for(setting, cause)
    ON[setting](scene)
    fields = None
    if cause != "solids":
        setup, _, fields = CAUSES[cause]
        if setup:
            setup(scene)
    r = _Renders(scene)
    return r.answers(fields), r.untouched()


@pytest.mark.parametrize("setting,cause", sorted(vr.RENDER_REFUSALS))
def test_a_render_is_refused_in_the_recorded_words(setting, cause):
    answers, untouched = render_answers(setting, cause)
    for status, message in answers:
        assert status == _lib.NT_E_UNSUPPORTED, (status, message)
        assert message == vr.RENDER_REFUSALS[setting, cause]
    assert untouched


def test_the_table_of_render_refusals_is_whole():
    count = {}
    for setting, cause in vr.RENDER_REFUSALS:
        count[setting] = count.get(setting, 0) + 1
    # (one less than the terms of whole_view_check: the row range cannot be reached through the ABI)
    assert count == {"ao": 5, "face lines": 5, "outlines": 6, "cue": 7, "clip": 9}
    assert len(set(vr.RENDER_REFUSALS.values())) == len(vr.RENDER_REFUSALS)


def precedence_answers(upper, lower):
    """the answers with both settings on, and with `upper` off again and a supersampling factor in the way of `lower`"""
    scene = _scene_for(upper)
    ON[upper](scene)
    ON[lower](scene)
    r = _Renders(scene)
    both = r.answers(None)
    OFF[upper](scene)
    scene.set_supersampling(2)
    return both, r.answers(None), r.untouched()


@pytest.mark.parametrize("upper,lower", [(u, l) for i, u in enumerate(COMPOSITE) for l in COMPOSITE[i + 1:]])
def test_of_two_settings_the_one_nearer_the_top_of_the_table_refuses(upper, lower):
    both, alone, untouched = precedence_answers(upper, lower)
    for status, message in both:
        assert status == _lib.NT_E_UNSUPPORTED and message == vr.RENDER_REFUSALS[upper, lower]
    for status, message in alone:
        assert status == _lib.NT_E_UNSUPPORTED and message == vr.RENDER_REFUSALS[lower, "supersampling"]
    assert untouched


# ------------------------------------------------------------------ the entry points that return a setting's buffer

# entry -> (the setting, bytes an element, the host form's arguments after the buffer)
ENTRIES = {
    "nt_adaptive_mask": ("adaptive", 1, (None,)),
    "nt_ambient_occlusion": ("ao", 4, ()),
    "nt_outline_mask": ("outlines", 1, (None,)),
    "nt_depth_cue_factors": ("cue", 8, ()),
    "nt_box_line_mask": ("face lines", 1, (None,)),
}
# the fields the device forms refuse, by the helper each of them asks
DEVICE_FIELDS = ("band_rank", "band_world", "band_rows", "compact", "collect_stats", "overlapped")


def _calls(entry):
    """(host form, device form), each (scene handle, w, h, buffer, options or None) -> status"""
    L = _lib.lib()
    extra = ENTRIES[entry][2]
    host = lambda s, w, h, p, o: getattr(L, entry)(s, w, h, p, *extra, o)
    devf = lambda s, w, h, p, o: getattr(L, entry + "_device")(s, w, h, p, o, None)
    return host, devf


def query_answers(entry, cause):
    """[(status, message)] of the host and the device form of `entry` with `cause` in the way, and whether the buffer is as it was;
    the causes "options: <field>" are the device form's alone"""
    setting, elem, _ = ENTRIES[entry]
    scene = _scene_for(setting)
    other = tracern.BoxScene(4) if setting != "face lines" else _scene_for("ao")
    ON[setting](scene)
    out = np.full(W * H * elem, 77, np.uint8)
    args, fields = [scene._handle, W, H, out.ctypes.data], None
    if cause == "NULL scene":
        args[0] = None
    elif cause == "NULL buffer":
        args[3] = None
    elif cause == "size":
        args[1] = 0
    elif cause == "scene kind":
        args[0] = other._handle
    elif cause == "clip":
        ON["clip"](scene)
    elif cause == "off":
        OFF[setting](scene)
    elif cause in ("lens", "parallel"):
        CAUSES[cause][0](scene)
    elif cause in ("bands", "collect_stats"):
        fields = CAUSES[cause][2]
    elif cause == "pixels":
        args[1], args[2] = 65536, 32768
    elif cause.startswith("options: "):
        fields = {cause[len("options: "):]: 1}
    else:
        raise KeyError(cause)
    opts = None if fields is None else sup.render_opts(**fields)
    forms = _calls(entry)
    if cause.startswith("options: "):
        forms = forms[1:]
    answers = []
    for call in forms:
        status = call(*args, None if opts is None else C.byref(opts))
        answers.append((status, _lib.last_error()))
    return answers, bool((out == 77).all())


@pytest.mark.parametrize("entry,cause", sorted(vr.QUERY_REFUSALS))
def test_an_entry_point_refuses_in_the_recorded_words(entry, cause):
    answers, untouched = query_answers(entry, cause)
    want_status, want = vr.QUERY_REFUSALS[entry, cause]
    assert answers
    for status, message in answers:
        assert (status, message) == (want_status, want)
    assert untouched


def test_the_table_of_entry_point_refusals_is_whole():
    common = {"NULL scene", "NULL buffer", "size", "off", "lens", "parallel"}
    options = {"options: " + f for f in DEVICE_FIELDS}
    want = {
        "nt_adaptive_mask": common | {"clip", "bands", "collect_stats"},
        "nt_ambient_occlusion": common | {"scene kind", "clip"} | options,
        "nt_outline_mask": common | {"scene kind", "clip"} | options,
        "nt_depth_cue_factors": common | {"scene kind", "clip"} | options,
        "nt_box_line_mask": common | {"scene kind", "pixels"} | options | {"options: strict_reference"},
    }
    got = {}
    for entry, cause in vr.QUERY_REFUSALS:
        got.setdefault(entry, set()).add(cause)
    assert got == want


# ------------------------------------------------------------------ what can only be read

def test_one_check_one_table_and_the_row_range_guard():
    with open(os.path.join(ROOT, "ntracer_amd", "csrc", "nt_api.cpp")) as f:
        api = f.read()
    # the row range is a guard for callers inside nt_api.cpp: the entry points hand over whole images unless band_world > 1,
    # which is refused first, so it can only be read, not reached
    assert api.count("int whole_view_check(") == 1
    assert "for a row range" in sup.function_body(api, "int whole_view_check(")
    for gone in ("ao_check", "outline_check", "box_lines_check", "cue_check", "clip_check"):
        assert gone not in api, gone
