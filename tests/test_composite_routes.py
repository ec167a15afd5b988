"""The kernel routes of tests/test_composite_matrix.py, pinned to the C++ that picks them: every hipLaunchKernelGGL of
launch_composite_fixed<N> (nt_composite.hpp) and nt_launch_composite (nt_var.hip) must have a row in
fixtures.COMPOSITE_ROUTES, and every NTRACER_* switch that read_switches (nt_api.cpp, the one place the render switches are
read) reads must be set by one of its ways, so that a kernel variant or a switch added later without a matrix row fails here,
without a GPU.  The two thresholds the deep-tree rows are built around are pinned as well."""
import os
import re

import fixtures as fx
import support as sup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ntracer_amd", "csrc")


def _fixed():
    return sup.function_body(sup.source("nt_composite.hpp"), "int launch_composite_fixed(")


def _var():
    return sup.function_body(sup.source("nt_var.hip"), "int nt_launch_composite(")


def _reader():
    return sup.function_body(sup.source("nt_api.cpp"), "RenderSwitches read_switches(")


def test_every_composite_launch_has_a_matrix_row():
    launched = sup.launches_through(sup.source("nt_composite.hpp"), "int launch_composite_fixed(") | sup.launches(_var())
    assert len(launched) >= 14, sorted(launched)            # the scan still finds the launches
    rows = [k for k, _ in fx.COMPOSITE_ROUTES]
    assert len(rows) == len(set(rows)), "duplicate rows"
    assert set(rows) == launched, ("launched without a row: %s; rows nothing launches: %s"
                                   % (sorted(launched - set(rows)), sorted(set(rows) - launched)))
    for kernel, ways in fx.COMPOSITE_ROUTES:
        assert ways, kernel
        for scene, params, env, mode in ways:
            assert scene in ("lean", "mixed", "deep"), (kernel, scene)
            assert params in ("unlit", "lit", "reflective", "transparent", "transparent_reflective"), (kernel, params)
            assert mode in ("render", "stats", "colors_at"), (kernel, mode)
            assert all(k.startswith("NTRACER_") for k in env), (kernel, env)


def test_every_composite_switch_the_reader_or_launchers_read_is_set_by_a_row():
    read = set(re.findall(r'getenv\("(NTRACER_\w+)"\)', _reader() + _fixed() + _var()))
    read -= {s for s in read if s.startswith("NTRACER_BOX_")}      # BoxScene's (read before the scene kind is known)
    assert {"NTRACER_COMPOSITE_KERNEL", "NTRACER_TWO_PASS", "NTRACER_FRAME_MAJOR"} <= read, sorted(read)
    set_by_rows = {k for _, ways in fx.COMPOSITE_ROUTES for _, _, env, _ in ways for k in env}
    set_by_rows |= {k for env in fx.COMPOSITE_FRAME_ENVS for k in env}
    assert read <= set_by_rows, "switches no matrix row sets: %s" % sorted(read - set_by_rows)


# every render switch read_switches reads, once each
RENDER_SWITCHES = ("NTRACER_STRICT_REFERENCE", "NTRACER_CLEAN_NORMALS", "NTRACER_FORCE_VAR", "NTRACER_COMPOSITE_KERNEL",
                   "NTRACER_NUMERATORS", "NTRACER_TWO_PASS", "NTRACER_TILE_ORDER", "NTRACER_FRAME_MAJOR", "NTRACER_CHUNK_FRAMES",
                   "NTRACER_BOX_CULL", "NTRACER_BOX_INTERLEAVE", "NTRACER_BOX_VAR_ROWS")


def test_the_reader_reads_exactly_the_render_switches_and_nothing_else_calls_getenv():
    """read_switches is the one place the render switches are read, and it reads each of RENDER_SWITCHES once and nothing
    else: no other code in csrc calls getenv, except the k-d builder for NTRACER_BUILD_THREADS (not a render switch)"""
    reader = re.findall(r"\bgetenv\s*\(([^)]*)\)", _reader())
    assert sorted(reader) == sorted('"%s"' % k for k in RENDER_SWITCHES), reader
    for name in sorted(os.listdir(CSRC)):
        calls = re.findall(r"\bgetenv\s*\(([^)]*)\)", sup.source(name))
        want = {"nt_api.cpp": reader, "nt_builder.cpp": ['"NTRACER_BUILD_THREADS"']}.get(name, [])
        assert calls == want, (name, calls)


def test_every_enqueue_takes_its_route_from_composite_route():
    """the host allocates the scratch the chosen kernel reads, so it must choose as the launchers do: the rule is written once, in
    composite_route, and the enqueues that size `checked` columns, frame stacks or the packet walk's scratch ask it and keep no
    terms of their own (enqueue_lens, enqueue_parallel and enqueue_ao: test_lens_host, test_parallel_host, test_ao_host)"""
    api = sup.source("nt_api.cpp")
    for head in ("int plan_composite(", "int hits_enqueue(", "int query_enqueue(", "int rays_scene("):
        start = api.rindex(head)                                      # (the definition: some are declared further up)
        body = sup.function_body(api[start:], head)
        assert body.count("\n") > 5 and "composite_route(" in body, head
        assert "all_opaque" not in body, head


def test_the_thresholds_the_deep_rows_are_built_around():
    fixed = _fixed()
    # the packet kernel takes trees of stack_depth <= 32 only: its uniform stack has 32 entries and a 32-bit `bothbits`
    assert re.search(r"li\.kernel_choice == 0 && sc\.stack_depth <= 32\)", fixed)
    # (launched as composite_packet<N, 32, ...>: DEPTH = 32, pinned by the rows' names)
    hpp = sup.source("nt_composite.hpp")
    assert re.search(r"if \(m_far != 0ull && sp < DEPTH\)", hpp)
    # the per-lane kernels' LDS: 256 lanes x (4 stack_depth + 8 N + 4 NT_MBOX) bytes, refused beyond 160 KiB -- four waves of
    # wave_lds_bytes, the function the kernels carve by, through lane_walk_lds, which holds the refusal
    assert re.search(r"if \(const int r = lane_walk_lds\(sc, N, 4, 160 \* 1024, lds\)\) return r;", fixed)
    per_wave = sup.function_body(hpp, "__host__ __device__ __forceinline__ size_t wave_lds_bytes(int stack_depth, int n)")
    assert re.search(r"return \(size_t\)64 \* \(\(size_t\)stack_depth \* 4 \+ \(size_t\)n \* 8 \+ \(size_t\)NT_MBOX \* 4\);", per_wave)
    walk = sup.function_body(hpp, "inline int lane_walk_lds(const NtCompositeDev &sc, int n, int waves, size_t limit, size_t &lds)")
    assert re.search(r"lds = \(size_t\)waves \* wave_lds_bytes\(sc\.stack_depth, n\);\s*if \(lds <= limit\) return 0;\s*"
                     r"snprintf\([^;]*\"k-d tree too deep for the LDS traversal stack \(depth %d\)\", sc\.stack_depth\);\s*return -1;", walk)
    assert re.search(r"#define NT_MBOX 16\b", hpp)
    # ... so the deepest tree that fits at N = 10 has stack_depth 124
    n, sd = 10, fx.COMPOSITE_MAX_DEPTH_N10
    assert 256 * (4 * sd + 8 * n + 64) == 160 * 1024
    # and the deep depths straddle the packet kernel's limit; 64 passes 64 KB of LDS at N >= 8
    assert min(fx.COMPOSITE_DEEP_DEPTHS) <= 31 and 32 in fx.COMPOSITE_DEEP_DEPTHS and 33 in fx.COMPOSITE_DEEP_DEPTHS
    assert all(256 * (4 * sd + 8 * 8 + 64) > 64 * 1024 for sd in fx.COMPOSITE_DEEP_DEPTHS_WIDE)
