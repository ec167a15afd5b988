"""The run-time-n CompositeScene kernels at n = 17 .. 64, the part that needs no GPU: the floors of every case of
tests/high_dimension_cases.py by the oracle alone (no case may pass on background), the arithmetic of the LDS sizes the cases
rest on, pinned to the C++ that computes them, the kernel pointer every launcher hands to var_walk_ready against the kernel it
then launches, and the route table: every run-time-n walk kernel has cases that tests/test_high_dimension_gpu.py runs, below
and above the 64 KiB at which a launch needs hipFuncAttributeMaxDynamicSharedMemorySize."""
import re

import numpy as np
import pytest

import high_dimension_cases as hd
import support as sup
from ntracer_amd import tracern

W, H = hd.VIEW

# which cases land on which member of a kernel family: the plain kernel, its _t<true> and its _t<false> form (scene, kind, clean)
PLAIN = [("wide", "unlit", False), ("wide", "lit", False), ("mixed", "lit", True)]
ALIASED = [("wide", "transparent_reflective", False), ("mixed", "lit", False), ("mixed", "transparent", False)]
CLEAN = [("mixed", "transparent", True)]
OPAQUE = [("wide", "unlit", False), ("wide", "lit", False), ("mixed", "lit", False), ("mixed", "lit", True)]
TRANSPARENT = [("wide", "transparent_reflective", False), ("mixed", "transparent", False), ("mixed", "transparent", True)]
FAMILIES = [("composite_kernel_var", ("render", "colors_at")), ("query_closest_var", ("intersect",)), ("hits_closest_var", ("primary_hits",)),
            ("rays_color_var", ("ray_colors",)), ("refine_color_var", ("refine",))]
HIGH_ROUTES = [(stem + suffix, calls, ways) for stem, calls in FAMILIES for suffix, ways in (("", PLAIN), ("_t<true>", ALIASED), ("_t<false>", CLEAN))]
HIGH_ROUTES += [("query_occluded_var", ("occludes",), OPAQUE), ("query_occluded_var_t", ("occludes",), TRANSPARENT)]
WALK_LAUNCHERS = ("nt_launch_composite", "nt_launch_query", "nt_launch_hits", "nt_launch_rays", "nt_launch_refine")


def _cases_of(way, call):
    scene, kind, clean = way
    pool = hd.refine_cases() if call == "refine" else hd.core_cases()
    return [c for c in pool if c[0] == scene and c[3] == kind and c[4] == clean]


# ------------------------------------------------------------------ floors
@pytest.mark.parametrize("case", hd.core_cases(), ids=hd.case_id)
def test_every_case_meets_its_floors_by_the_oracle_alone(case):
    hd.check_case(case)
    fr, r = hd.frame(case), hd.rays(case)
    print("%s: %d of %d primary rays hit, %d shadow rays, %d rays; of the %d ray-lattice rays %d hit, %d are blocked, %d pass something transparent"
          % (hd.case_id(case), fr.counters["hits"], W * H, fr.counters["shadow_rays"], fr.counters["rays"], len(r.origins),
             int((r.closest["item"] >= 0).sum()), int(r.blocked["blocked"].sum()), int((r.closest["n_transparent"] > 0).sum())))


@pytest.mark.parametrize("n", hd.MIXED_DIMS)
def test_the_normal_modes_of_the_mixed_scene_differ(n):
    hd.check_normal_modes(n)
    for kind in hd.MIXED_KINDS:
        print("mixed(%d) %s: the normal modes differ on %r" % (n, kind, hd.normal_mode_counts(n, kind)))
    flat = hd.mixed(n)
    assert len(flat["batch_recs"]) == 2 and len(flat["tri_recs"]) == 4
    assert list(flat["solid_types"]) == [tracern.CUBE, tracern.SPHERE, tracern.CUBE]
    # the grafted root: a cut on axis 2 whose near child is the leaf of the sphere and the second cube
    root = int(flat["root"])
    assert flat["node_axis"][root] == 2 and abs(float(flat["node_split"][root]) - hd.FRONT_CUT) < 1e-6
    leaf = int(flat["node_left"][root])
    assert flat["node_axis"][leaf] == -1 and sorted(int(i) >> 2 for i in flat["items"][flat["node_left"][leaf]:][:2]) == [1, 2]


@pytest.mark.parametrize("case", hd.refine_cases(), ids=hd.case_id)
def test_the_refine_cases_flag_some_pixels_and_leave_others(case):
    hd.check_refine(case)


@pytest.mark.parametrize("case", hd.SETTING_CASES, ids=hd.case_id)
def test_the_five_settings_show_on_the_small_view(case):
    hd.check_settings(case)
    c = hd.settings(case)
    assert c.origin[63] != 0 and c.cue["tint_axis"][63] != 0 and (c.ao_table != 0).all() and c.ao_table.shape == (hd.AO_K, 64)


@pytest.mark.parametrize("case", hd.limit_cases(), ids=hd.case_id)
def test_the_deepest_scene_that_fits_shows_its_four_batches(case):
    s, fr = hd.scene(case), hd.frame(case)
    hd.check_scene(s.flat)
    assert s.stack_depth == hd.MAX_DEPTH_N64 and s.lds == hd.LDS_LIMIT
    cnt = fr.counters
    # (the unlit render sends primary rays alone: its `hits` are the pixels that show something)
    primary = hd.frame(case[:3] + ("unlit", False)).counters
    assert primary["rays"] == W * H and primary["hits"] * 4 >= W * H and (W * H - primary["hits"]) * 10 >= W * H, primary
    assert len(np.unique(np.asarray(fr.frame).reshape(-1, 3), axis=0)) > 50
    if hd.is_lit(case[3]):
        assert cnt["shadow_rays"] > 0
    if hd.is_transparent(case[3]):
        assert cnt["rays"] > W * H
    # every primary ray crosses every split inside the box: the walk pushes stack_depth - 2 entries
    assert fr.centre["branches"] == hd.MAX_DEPTH_N64 - 2, fr.centre


def test_face_normals_of_every_scene_are_far_from_underflow_and_the_old_combs_are_not():
    for n, depth in hd.DIMS:
        ln = hd.face_normal_lengths(hd.wide_comb(n, depth))
        assert (ln >= 1e-20).all() and (ln <= 1e20).all(), (n, depth, float(ln.min()), float(ln.max()))
    # the trap this module's scenes avoid: comb_flat's edges of 0.044 .. 0.088 give a face normal of exactly 0 in fp32 at n = 33
    import test_composite_matrix as tcm
    assert hd.face_normal_lengths(tcm.comb_flat(33, 3)).max() < 1e-20


# ------------------------------------------------------------------ the arithmetic the cases rest on
def test_lds_sizes_of_the_cases():
    assert hd.lds_bytes(59, 4) == 65536 == hd.LDS_ATTRIBUTE
    assert hd.lds_bytes(59, 5) == 65792
    assert hd.lds_bytes(64, 368) == 163840 == hd.LDS_LIMIT
    assert hd.lds_bytes(64, 369) == 164096
    assert hd.lds_bytes(60, 2) > hd.LDS_ATTRIBUTE                  # n >= 60: at any depth
    for n, depth in hd.DIMS:
        s = hd.scene(("wide", n, depth, "unlit", False))
        assert s.stack_depth == depth and s.lds == hd.lds_bytes(n, depth)
    below = [(n, d) for n, d in hd.DIMS if hd.lds_bytes(n, d) <= hd.LDS_ATTRIBUTE]
    above = [(n, d) for n, d in hd.DIMS if hd.lds_bytes(n, d) > hd.LDS_ATTRIBUTE]
    assert below == [(17, 4), (33, 4), (59, 4)] and above == [(59, 5), (60, 3), (64, 4)]
    assert hd.scene(("mixed", 17, None, "lit", False)).lds <= hd.LDS_ATTRIBUTE < hd.scene(("mixed", 64, None, "lit", False)).lds
    assert hd.stack_depth_of(hd.wide_comb(64, hd.MAX_DEPTH_N64 + 1, [0])) == hd.MAX_DEPTH_N64 + 1


def test_var_lds_bytes_is_that_expression_and_the_limits_are_where_the_cases_put_them():
    src = sup.source("nt_var.hip")
    body = sup.function_body(src, "__host__ __device__ __forceinline__ size_t var_lds_bytes(int depth, int n)")
    assert re.search(r"return \(size_t\)64 \* \(\(size_t\)n \* 16 \+ \(size_t\)depth \* 4 \+ \(size_t\)NT_MBOX \* 4\);", body), body
    mbox = re.search(r"#define\s+NT_MBOX\s+(\d+)", sup.source("nt_composite.hpp") + sup.source("nt_device.hpp"))
    assert mbox and int(mbox.group(1)) == 16                        # 64 bytes a lane
    ready = sup.function_body(src, "int var_walk_ready(")
    assert re.search(r"lds = var_lds_bytes\(sc\.stack_depth, n\);", ready)
    assert re.search(r"if \(lds > 160 \* 1024\) \{\s*snprintf\([^;]*\"scene too deep for the LDS budget \(n %d, depth %d\)\", n, sc\.stack_depth\);\s*return -1;", ready), ready
    assert re.search(r"if \(lds > 64 \* 1024\) \(void\)hipFuncSetAttribute\(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, \(int\)lds\);", ready), ready
    # the refusal comes before the attribute, and the launchers launch nothing before var_walk_ready has answered
    assert ready.index("160 * 1024") < ready.index("hipFuncSetAttribute")
    for head in WALK_LAUNCHERS:
        b = sup.function_body(src, "int %s(" % head)
        first = min(m.start() for m in re.finditer(r"hipLaunchKernelGGL\(\s*\w*(?:composite_kernel|query_|hits_|rays_color|refine_color)\w*_var", b))
        assert b.index("var_walk_ready(") < first, head
    assert "std::max(s->depth + 1, 2)" in sup.function_body(sup.source("nt_api.cpp"), "void fill_composite(")


def _named_kernels(body):
    """the kernels a launcher names for var_walk_ready: both members of every alias_kernel pair and every kernel cast to a pointer"""
    names = set()
    for a, b in re.findall(r"alias_kernel\(\*?sc,\s*([\w<>]+),\s*([\w<>]+)\)", body):
        names |= {a, b}
    names |= set(re.findall(r"reinterpret_cast<const void \*>\((\w+)\)", body))
    return names


def _lds_launches(body):
    """the kernels a launcher launches with the dynamic LDS var_walk_ready sized (BoxScene's kernels size their own: no walk)"""
    names = re.findall(r"hipLaunchKernelGGL\(\s*([A-Za-z_]\w*(?:<[^<>]*>)?)\s*,[^;]*?,\s*lds\s*,", body)
    return {n for n in names if "_box_" not in n}


def test_every_launcher_hands_var_walk_ready_the_kernels_it_launches():
    src = sup.source("nt_var.hip")
    launchers = [h for h in re.findall(r"\nint (nt_launch_\w+)\(", src) if "var_walk_ready(" in sup.function_body(src, "int %s(" % h)]
    assert sorted(launchers) == sorted(WALK_LAUNCHERS)
    union = set()
    for head in launchers:
        body = sup.function_body(src, "int %s(" % head)
        named, launched = _named_kernels(body), _lds_launches(body)
        assert named and named == launched, (head, sorted(named - launched), sorted(launched - named))
        assert launched <= sup.launches(body)
        # every var_walk_ready of the launcher takes a kernel the launcher names, never a null or a cached pointer
        for arg in re.findall(r"var_walk_ready\(li\.n, \*?sc, (.*?), lds\)", body):
            assert arg == "kernel" or arg.startswith("alias_kernel(") or arg.startswith("reinterpret_cast<const void *>("), (head, arg)
        # within a pair the launch picks on the flag alias_kernel picks on
        for a, b in re.findall(r"alias_kernel\(\*?sc,\s*([\w<>]+),\s*([\w<>]+)\)", body):
            assert a.endswith("<true>") and b.endswith("<false>") and a[:-6] == b[:-7], (head, a, b)
            assert re.search(r"if \(sc(?:\.|->)alias_normals\)\s*hipLaunchKernelGGL\(%s," % re.escape(a), body), (head, a)
            assert re.search(r"else\s+hipLaunchKernelGGL\(%s," % re.escape(b), body), (head, b)
        union |= launched
    assert "return reinterpret_cast<const void *>(sc.alias_normals ? aliased : clean);" in src
    assert union == set(hd.KERNELS), (sorted(union - set(hd.KERNELS)), sorted(set(hd.KERNELS) - union))


# ------------------------------------------------------------------ routes
def test_every_walk_kernel_has_cases_below_and_above_64_kib():
    rows = [k for k, _, _ in HIGH_ROUTES]
    assert len(rows) == len(set(rows)) and set(rows) == set(hd.KERNELS)
    reached = {}
    for kernel, calls, ways in HIGH_ROUTES:
        for call in calls:
            assert call in hd.CALLS
            for way in ways:
                cases = _cases_of(way, call)
                if call == "refine" and not cases:           # (one opaque and one transparent refine case per n, not every kind)
                    continue
                assert cases, (kernel, call, way)
                for case in cases:
                    assert hd.route(case, call) == kernel, (kernel, call, case, hd.route(case, call))
                    reached.setdefault(kernel, []).append(hd.scene(case).lds)
    # and no call of any case lands on a kernel without a row
    for case in hd.core_cases():
        for call in hd.CALLS[:-1]:
            assert hd.route(case, call) in reached
    for kernel in hd.KERNELS:
        sizes = reached[kernel]
        assert min(sizes) <= hd.LDS_ATTRIBUTE < max(sizes) <= hd.LDS_LIMIT, (kernel, sorted(set(sizes)))
    # the rule itself: composite_route's `faithful` and `var` (nt_api.cpp)
    api = sup.source("nt_api.cpp")
    assert "r.faithful = !s->all_opaque || (s->n_solids > 0 && !sw.clean_normals);" in api
    assert "r.var = s->n > NT_MAX_FIXED_DIM || sw.force_var;" in api and "c.alias_normals = sw.clean_normals ? 0 : 1;" in api


def test_dimension_65_is_refused_as_the_box_scene_refuses_it():
    n = 65
    rl = n * n + n + 1
    d = dict(hd.wide_comb(64, 3, [0]))
    d.update(batch_recs=np.zeros((1, 4, rl), np.float32), tri_recs=np.zeros((0, rl), np.float32), solid_recs=np.zeros((0, 2 * n * n + n), np.float32),
             aabb_start=np.full(n, -1, np.float32), aabb_end=np.full(n, 1, np.float32))
    with pytest.raises(ValueError, match="dimension"):
        tracern.CompositeScene.from_flat(n, d)
    with pytest.raises(ValueError, match="dimension"):
        tracern.BoxScene(n)
    assert tracern.CompositeScene.from_flat(64, hd.wide_comb(64, 3, [0])).dimension == 64
