"""Shared helpers for the tests: fixture loading (tests/golden/*.npz are DATA captured from the compiled
reference by tools/gen_golden.py)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

FLAT_KEYS = ("root", "node_axis", "node_split", "node_left", "node_right", "items", "batch_recs", "batch_mats",
             "tri_recs", "tri_mats", "solid_recs", "solid_types", "solid_mats", "materials", "aabb_start", "aabb_end")
PARAM_KEYS = ("fov", "shadows", "camera_light", "max_reflect_depth", "bg_gradient_axis", "ambient", "bg1", "bg2",
              "bg3", "point_light_pos", "point_light_color", "global_light_dir", "global_light_color")
RGBX8 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1), (8, 0, 0, 0)]
RGB16 = [(16, 1, 0, 0), (16, 0, 1, 0), (16, 0, 0, 1)]
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]

BOX_FIXTURES = ["box_n3_1920x1080", "box_n6_1920x1080", "box_n10_4096x4096", "box_n6_640x480_generic",
                "box_n5_320x200", "box_n8_320x200", "box_n12_320x200"]


# BoxScene's fused tile kernel (box_tile_kernel, ntracer_amd/csrc/nt_box.hpp): launches that land on each block shape
# nt_box_tile_geom (nt_device.hpp) picks and on each split of the redo kernel (N >= 9, packed RGB), in the order
# tests/test_box_tile_matrix.py runs them (the scratch buffers grow, then are reused by smaller launches).
# (width, height, frames, (rows a wave, waves a block), redo split, bytes of pitch padding)
BOX_TILE_SHAPES = [
    (640, 360, 40, (8, 4), 2, 0),          # small multi-frame launch with lead frames
    (1920, 1000, 40, (16, 3), 2, 64),      # three waves a block
    (1920, 1080, 72, (64, 1), 1, 0),       # the bench's shape
    (4100, 520, 60, (64, 1), 1, 64),       # three redo words a row (> 2048 pixels)
    (1000, 700, 100, (16, 4), 1, 64),      # split 1 with 16-row waves, ragged last column
    (1930, 1080, 17, (16, 4), 2, 0),       # ragged last column, no lead frames
]
# one rank's bands of the bench's call: (width, height, frames, band_rank, band_world, band_rows, (rows, waves), split);
# compact buffer, 136 owned rows
BOX_TILE_BAND = (1920, 1080, 160, 3, 8, 8, (16, 3), 2)


def box_redo_split(width, row_count, frames):
    """launch_box_fixed's choice between box_redo_kernel<N, 2> (two waves a redo word) and <N, 1>"""
    redo_words = ((width + 63) // 64 + 31) // 32
    return 2 if row_count * frames * redo_words < 48 * 1024 else 1


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def flat_of(g, opaque=False):
    flat = {k: g[k] for k in FLAT_KEYS}
    flat["batch_size"] = 4
    if opaque:
        m = np.array(g["materials"], np.float32).copy()
        m[:, 6] = 1.0
        flat["materials"] = m
    return flat


def params_of(g, prefix=""):
    return {k: g[prefix + k] for k in PARAM_KEYS}


def known_answer():
    with open(os.path.join(GOLDEN, "kdtree_known_answer.json")) as f:
        return json.load(f)


def known_answer_flat(ka):
    """Flatten the hand-built scene of the reference's test_kdtree into the nt_scene_desc layout."""
    n = ka["dimension"]
    recs = []
    for t in ka["triangles"]:
        fn = np.asarray(t["face_normal"], np.float32)
        p1 = np.asarray(t["p1"], np.float32)
        d = np.float32(0)
        acc = np.float32(fn[0] * p1[0])
        for k in range(1, n):
            acc = np.float32(acc + np.float32(fn[k] * p1[k]))
        d = -acc
        rec = [d] + list(fn) + list(p1)
        for e in t["edge_normals"]:
            rec += list(np.asarray(e, np.float32))
        recs.append(rec)
    nodes, items = [], []

    def add(node):
        if node is None:
            return -1
        idx = len(nodes)
        nodes.append(None)
        if "leaf" in node:
            start = len(items)
            items.extend((i << 2) | 1 for i in node["leaf"])
            nodes[idx] = (-1, 0.0, start, len(node["leaf"]))
        else:
            b = node["branch"]
            l = add(b["left"])
            r = add(b["right"])
            nodes[idx] = (b["axis"], b["split"], l, r)
        return idx

    root = add(ka["tree"])
    nd = np.asarray(nodes, np.float64)
    rl = n * n + n + 1
    return dict(root=root, node_axis=nd[:, 0].astype(np.int32), node_split=nd[:, 1].astype(np.float32),
                node_left=nd[:, 2].astype(np.int32), node_right=nd[:, 3].astype(np.int32),
                items=np.asarray(items, np.int32), batch_recs=np.zeros((0, 4, rl), np.float32),
                batch_mats=np.zeros((0, 4), np.int32), tri_recs=np.asarray(recs, np.float32),
                tri_mats=np.zeros(len(recs), np.int32), solid_recs=np.zeros((0, 2 * n * n + n), np.float32),
                solid_types=np.zeros(0, np.int32), solid_mats=np.zeros(0, np.int32),
                materials=np.asarray([[1, 1, 1, 1, 1, 1, 1, 0, 1, 8]], np.float32),
                aabb_start=np.asarray(ka["aabb"]["start"], np.float32), aabb_end=np.asarray(ka["aabb"]["end"], np.float32),
                batch_size=4)


def stress_cameras(n, rng):
    """orientations x origins chosen to land rays on edges, faces' planes, the inside, grazing directions"""
    cams = []
    eye = np.eye(n, dtype=np.float32)
    for k in range(10):
        q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        if k == 0:
            q = eye.copy()                                   # axis-aligned: direction components exactly 0
        elif k == 1:
            q = eye + 1e-7 * rng.standard_normal((n, n))     # almost axis-aligned: grazing rays
        elif k == 2:
            q = eye[rng.permutation(n)]
        elif k == 3:
            q = q.copy()
            q[1] = q[1] + 0.8 * q[2] + 0.3 * q[0]            # `up` far from orthogonal: no quadratic |dir|^2 shortcut
        elif k == 4:
            q = q.copy()
            q[0] = 3.0 * q[0]                                # stretched `right`
            q[1] = 0.0 * q[1]                                # ... and no `up` at all: every row the same
        q = np.ascontiguousarray(q, np.float32)
        for dist in (0.3, 1.0, 1.0000001, 1.7, 3.0, 9.0, 60.0):
            back = -q[2] * np.float32(dist)                  # look at the centre from `dist` away ...
            cams.append((back.astype(np.float32), q))
            off = back + np.float32(0.4) * q[0] + np.float32(0.25) * q[1]          # ... and off-centre
            cams.append((off.astype(np.float32), q))
        o = np.zeros(n, np.float32)
        o[:3] = (-1.0, 0.3, -2.5)                            # origin exactly on the plane of a face
        cams.append((o, q))
        o = o.copy()
        o[0] = 1.0
        o[min(3, n - 1)] = 1.0                               # on two planes at once
        cams.append((o, q))
    return cams


def diagonal_camera(n, dist, rng):
    """tools/box_soak.py's diagonal camera: every coordinate of the origin equal, looking at the centre -- whole regions of
    near-ties between faces"""
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    q = np.array(q, np.float32)
    o = np.full(n, -dist / np.sqrt(n), np.float32)
    q[2] = -o / np.linalg.norm(o)
    return o, np.ascontiguousarray(q, np.float32)


# CompositeScene's kernel routes (launch_composite_fixed<N> in ntracer_amd/csrc/nt_composite.hpp, nt_launch_composite in
# nt_var.hip), in the order tests/test_composite_matrix.py renders them at every fixed N = 3..10.  Each entry is one kernel
# instantiation as its hipLaunchKernelGGL spells it (spaces dropped), with the ways to reach it:
# (scene, parameter set, NTRACER_* switches, mode).  Scenes: "lean" (the N-orthoplex in batches), "mixed" (the same with four
# loose triangles, a cube and a sphere), "deep" (hand-built combs of stack_depth 31, 32, 33, 40, ...).  Modes: "render" (a
# 97 x 61 RGBF32 frame), "stats" (collect_stats=True) and "colors_at" (a pixel lattice).  tests/test_composite_routes.py
# checks, without a GPU, that every launch of the two functions and every non-BoxScene NTRACER_* switch has a row here.
COMPOSITE_ROUTES = [
    ("composite_packet<N,32,false,false>", [
        ("lean", "unlit", {}, "render"),
        ("lean", "unlit", {"NTRACER_NUMERATORS": "0", "NTRACER_TILE_ORDER": "0"}, "render"),
        ("lean", "unlit", {"NTRACER_STRICT_REFERENCE": "1"}, "render"),
        ("lean", "lit", {}, "render"),
        ("lean", "reflective", {}, "render"),
        ("deep", "unlit", {}, "render"),            # stack_depth <= 32
    ]),
    ("packet_numerators<N>", [
        ("lean", "unlit", {}, "render"),
    ]),
    ("composite_packet<N,32,true,false>", [
        ("lean", "lit", {"NTRACER_TWO_PASS": "0"}, "render"),
        ("lean", "reflective", {"NTRACER_TWO_PASS": "0"}, "render"),
    ]),
    ("composite_packet<N,32,false,true>", [
        ("mixed", "lit", {"NTRACER_CLEAN_NORMALS": "1"}, "render"),
    ]),
    ("composite_kernel<N,true,false,false>", [
        ("lean", "lit", {}, "render"),               # second pass of the two
        ("lean", "reflective", {}, "render"),
        ("lean", "lit", {"NTRACER_COMPOSITE_KERNEL": "2"}, "render"),
        ("lean", "lit", {}, "colors_at"),
        ("deep", "lit", {}, "render"),               # alone past stack_depth 32
    ]),
    ("composite_kernel<N,true,false>", [
        ("mixed", "lit", {"NTRACER_CLEAN_NORMALS": "1"}, "render"),
        ("mixed", "lit", {"NTRACER_CLEAN_NORMALS": "1", "NTRACER_COMPOSITE_KERNEL": "2"}, "render"),
    ]),
    ("composite_persistent<N>", [
        ("lean", "unlit", {"NTRACER_COMPOSITE_KERNEL": "1"}, "render"),
        ("deep", "unlit", {}, "render"),            # kernel choice 0 past stack_depth 32
        ("deep", "unlit", {"NTRACER_COMPOSITE_KERNEL": "1"}, "render"),
    ]),
    ("composite_kernel<N,false,false>", [
        ("lean", "unlit", {"NTRACER_COMPOSITE_KERNEL": "2"}, "render"),
        ("lean", "unlit", {}, "colors_at"),
        ("deep", "unlit", {"NTRACER_COMPOSITE_KERNEL": "2"}, "render"),
    ]),
    ("composite_kernel<N,true,true>", [
        ("lean", "unlit", {}, "stats"),
        ("mixed", "lit", {}, "stats"),              # the counting launch beside composite_kernel_t<N,true>
    ]),
    ("composite_kernel_t<N,true>", [
        ("mixed", "lit", {}, "render"),             # Solids: the reference's normal aliasing
        ("mixed", "lit", {}, "colors_at"),
        ("lean", "transparent", {}, "render"),
        ("lean", "transparent", {}, "colors_at"),
        ("mixed", "transparent", {}, "render"),
        ("deep", "transparent", {}, "render"),
    ]),
    ("composite_kernel_t<N,false>", [
        ("lean", "transparent", {"NTRACER_CLEAN_NORMALS": "1"}, "render"),
        ("mixed", "transparent", {"NTRACER_CLEAN_NORMALS": "1"}, "render"),
    ]),
    ("composite_kernel_var_t<true>", [
        ("lean", "transparent_reflective", {}, "render"),     # max_reflect_depth 6: more frames than NT_TFRAMES
        ("mixed", "lit", {"NTRACER_FORCE_VAR": "1"}, "render"),
    ]),
    ("composite_kernel_var_t<false>", [
        ("lean", "transparent_reflective", {"NTRACER_CLEAN_NORMALS": "1"}, "render"),
    ]),
    ("composite_kernel_var", [
        ("lean", "unlit", {"NTRACER_FORCE_VAR": "1"}, "render"),
        ("mixed", "lit", {"NTRACER_FORCE_VAR": "1", "NTRACER_CLEAN_NORMALS": "1"}, "render"),
    ]),
]
# the multi-frame launches of tests/test_composite_matrix.py (three frames through nt_render_frames_device at N = 6 and 9)
COMPOSITE_FRAME_ENVS = [{}, {"NTRACER_CHUNK_FRAMES": "2"}, {"NTRACER_FRAME_MAJOR": "0"}]
# stack_depth of the deep combs: around the packet kernel's 32-entry stack at every N, and beyond 64 KB of LDS at N >= 8
# (launch_composite_fixed: 256 * (4 * stack_depth + 8 * N + 64) bytes)
COMPOSITE_DEEP_DEPTHS = (31, 32, 33, 40)
COMPOSITE_DEEP_DEPTHS_WIDE = (64,)          # N = 8..10
COMPOSITE_MAX_DEPTH_N10 = 124               # 160 KiB at N = 10; one more is refused


def composite_route_ways():
    """the distinct (scene, params, env, mode) of COMPOSITE_ROUTES, in table order"""
    seen, out = set(), []
    for _, ways in COMPOSITE_ROUTES:
        for scene, params, env, mode in ways:
            key = (scene, params, tuple(sorted(env.items())), mode)
            if key not in seen:
                seen.add(key)
                out.append((scene, params, dict(env), mode))
    return out
