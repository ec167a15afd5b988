"""Primary-hit buffers (nt_primary_hits, nt_primary_hits_device, nt_primary_hits_table_device, CompositeScene.primary_hits)
against the oracle: every pixel of every view is compared with the record tests/primary_hit_cases.py works out for it --
nto_primary_dir, the fp32 restatement of aabb_distance, nto_kd_intersects -- none is left out.

item, lane and n_transparent must be equal for every pixel; dist and both normal arrays bitwise equal: the arithmetic
contract predicts a difference of 0, and DESIGN.md 4.4 measured 0 for these same walks and hit_normal.  Every record of the
image must be written and nothing else: the device buffers are prefilled with a sentinel, and the records between frames,
the records past the end and the normal rows of pixels without an opaque hit must still hold it.

Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import oracle_binding as ob
import primary_hit_cases as ph
import ray_query_cases as rq
import support as sup
from ntracer_amd import Material, _lib, render, tracern
from ntracer_amd.wrapper import NTracer

pytestmark = pytest.mark.gpu

FLT_MAX = ph.FLT_MAX
SENTINEL = 0x5a5a5a5a           # records
NSENTINEL = 7.0                 # normal rows
PAD = 5                         # records (and normal rows) behind the last frame

bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def _scene(case, mp, k=0):
    name, env = case
    sup.set_switches(mp, ph.SWITCHES, env)
    g, n, flat = rq.scene(name)
    sc = tracern.CompositeScene.from_flat(n, flat)
    sc.set_fov(ph.fov_of(name))
    sc._set_camera_arrays(*ph.camera(name, k))
    return sc


def _check(got, exp, label, normals=True):
    """got: dist / item / lane / n_transparent [H][W] and the two normal arrays; exp: primary_hit_cases.expected"""
    for key in ("item", "lane", "n_transparent"):
        bad = np.argwhere(np.asarray(got[key]) != exp[key])
        assert len(bad) == 0, "%s: %s differs on %d pixels, first (y, x) = %r: got %r, oracle %r" % (
            label, key, len(bad), tuple(bad[0]), np.asarray(got[key])[tuple(bad[0])], exp[key][tuple(bad[0])])
    bad = np.argwhere(bits(got["dist"]) != bits(exp["dist"]))
    assert len(bad) == 0, "%s: dist differs on %d pixels, first (y, x) = %r: got %r, oracle %r" % (
        label, len(bad), tuple(bad[0]), got["dist"][tuple(bad[0])], exp["dist"][tuple(bad[0])])
    if normals:
        hit = exp["item"] >= 0
        for key, ekey in (("normal_origin", "normal_origin"), ("normal_dir", "normal")):
            g, e = np.asarray(got[key])[hit], exp[ekey][hit]
            worst = float(np.abs(g.astype(np.float64) - e).max()) if hit.any() else 0.0
            assert np.array_equal(bits(g), bits(e)), "%s: %s differs on pixels with a hit, largest difference %g" % (label, key, worst)


def _device_pass(sc, n, w, h, normals, table=None, first=0, count=1, stride=None):
    """the _device forms through the ABI on sentinel-filled buffers with PAD records behind the last frame: (hits, normal
    origins, normal directions) as numpy arrays, padding included"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    stride = w * h if stride is None else stride
    total = count * stride + PAD
    hits = torch.full((total, 4), SENTINEL, dtype=torch.int32, device=dev)
    no = torch.full((total, n), NSENTINEL, dtype=torch.float32, device=dev) if normals else None
    nd = torch.full((total, n), NSENTINEL, dtype=torch.float32, device=dev) if normals else None
    res = _lib.NtHitBuffers()
    res.hits = hits.data_ptr()
    res.normal_origin, res.normal_dir = (no.data_ptr(), nd.data_ptr()) if normals else (None, None)
    opts = _lib.NtRenderOpts()
    opts.device = dev.index
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = _lib.lib()
    if table is None:
        _lib.check(L.nt_primary_hits_device(sc._handle, w, h, C.byref(res), C.byref(opts), stream))
    else:
        _lib.check(L.nt_primary_hits_table_device(sc._handle, w, h, C.byref(res), stride, table._h, first, count, C.byref(opts), stream))
    torch.cuda.synchronize()
    return hits.cpu().numpy(), (no.cpu().numpy() if normals else None), (nd.cpu().numpy() if normals else None)


def _frame(hits, no, nd, f, stride, w, h):
    """frame f of the raw buffers as _check wants it"""
    r = hits[f * stride:f * stride + w * h].reshape(h, w, 4)
    out = dict(dist=r[..., 0].view(np.float32), item=r[..., 1], lane=r[..., 2], n_transparent=r[..., 3])
    if no is not None:
        out["normal_origin"] = no[f * stride:f * stride + w * h].reshape(h, w, -1)
        out["normal_dir"] = nd[f * stride:f * stride + w * h].reshape(h, w, -1)
    return out


def _untouched(hits, no, nd, exp_items, stride, w, h, label):
    """the records between the frames and past the end, and the normal rows of every record that is no opaque hit, still hold
    the sentinel; exp_items: the expected item arrays of the frames"""
    count = len(exp_items)
    written = np.zeros(len(hits), bool)
    hit = np.zeros(len(hits), bool)
    for f, item in enumerate(exp_items):
        written[f * stride:f * stride + w * h] = True
        hit[f * stride:f * stride + w * h] = item.ravel() >= 0
    assert len(hits) == count * stride + PAD
    assert (hits[~written] == SENTINEL).all(), "%s: a record outside the frames was written" % label
    assert not (hits[written] == SENTINEL).all(axis=1).any(), "%s: a record of the image was not written" % label
    if no is not None:
        for key, a in (("normal_origin", no), ("normal_dir", nd)):
            assert (a[~hit] == NSENTINEL).all(), "%s: a %s row of a pixel without an opaque hit was written" % (label, key)


@pytest.mark.parametrize("case", ph.CASES, ids=ph.case_id)
def test_hits_equal_the_oracle(case):
    name, env = case
    g, n, flat = rq.scene(name)
    # ---- floors, by the oracle alone, so that no case can pass on all misses
    big = ph.expected(case, 64, 48)
    assert (big["item"] >= 0).sum() >= 40 and (big["item"] < 0).sum() >= 40, name
    if name in ("feature5_n5", "feature11_n11"):
        assert (big["n_transparent"] > 0).sum() >= 40, name
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        for w, h in ph.SIZES:
            label = "%s %dx%d" % (ph.case_id(case), w, h)
            exp = ph.expected(case, w, h)
            # ---- the host form through the Python surface
            got = sc.primary_hits(w, h, normals=True)
            assert got.dist.shape == (h, w) and got.normal_origin.shape == (h, w, n)
            _check(dict(dist=got.dist, item=got.item, lane=got.lane, n_transparent=got.n_transparent, normal_origin=got.normal_origin,
                        normal_dir=got.normal_dir), exp, label + " host")
            miss = exp["item"] < 0
            assert not got.normal_origin[miss].any() and not got.normal_dir[miss].any(), label         # (rows left as they were: zero)
            assert (got.kind[miss] == -1).all() and (got.index[miss] == -1).all()
            assert np.array_equal(got.kind[~miss], exp["item"][~miss] & 3) and np.array_equal(got.index[~miss], exp["item"][~miss] >> 2)
            plain = sc.primary_hits(w, h)
            assert plain.normal_origin is None and np.array_equal(plain.hits, got.hits), label
            # ---- the _device form on sentinel-filled buffers: bit for bit the host form's, and nothing else written
            hits, no, nd = _device_pass(sc, n, w, h, True)
            assert np.array_equal(hits[:w * h], got.hits), label + ": host and _device records differ"
            hitrows = ~miss.ravel()
            assert np.array_equal(bits(no[:w * h][hitrows]), bits(got.normal_origin.reshape(-1, n)[hitrows])), label
            assert np.array_equal(bits(nd[:w * h][hitrows]), bits(got.normal_dir.reshape(-1, n)[hitrows])), label
            _untouched(hits, no, nd, [exp["item"]], w * h, w, h, label)
            hits2, _, _ = _device_pass(sc, n, w, h, False)
            assert np.array_equal(hits2, hits), label + ": the records depend on whether normals were asked for"


@pytest.mark.parametrize("case", [("cell600_n4", {}), ("cell600_n4", {"NTRACER_CHUNK_FRAMES": "1"}), ("feature5_n5", {})], ids=ph.case_id)
def test_frames_of_a_camera_table(case):
    """three golden cameras in a table, frames [1, 3) of it in one launch, more than a frame's records between the frames: the
    packet walk, the packet walk a frame a chunk (launch_hits_fixed's own loop: the offsets of the second chunk into the
    records, the cameras and the numerator scratch) and a per-lane walk"""
    import torch
    name, env = case
    g, n, flat = rq.scene(name)
    w, h = 37, 21
    stride = w * h + 13
    cams = [ph.camera(name, k) for k in range(3)]
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        table = render.CameraTable(n, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
        hits, no, nd = _device_pass(sc, n, w, h, True, table, 1, 2, stride)
        exps = [ph.expected(case, w, h, k) for k in (1, 2)]
        assert not np.array_equal(exps[0]["item"], exps[1]["item"])                # (two different views)
        for f, exp in enumerate(exps):
            _check(_frame(hits, no, nd, f, stride, w, h), exp, "%s table frame %d" % (ph.case_id(case), 1 + f))
        _untouched(hits, no, nd, [e["item"] for e in exps], stride, w, h, ph.case_id(case) + " table")
        # the Python form: [count][H][W] views of tensors that stay on the device
        got = sc.primary_hits(w, h, normals=True, table=table, first=1, count=2, frame_stride=stride)
        assert got.item.is_cuda and tuple(got.item.shape) == (2, h, w) and tuple(got.normal_dir.shape) == (2, h, w, n)
        torch.cuda.synchronize()
        for f, exp in enumerate(exps):
            _check({k: getattr(got, k)[f].cpu().numpy() for k in ("dist", "item", "lane", "n_transparent", "normal_origin", "normal_dir")},
                   exp, "%s python table frame %d" % (ph.case_id(case), 1 + f))
        # what the ABI refuses about a table
        res = _lib.NtHitBuffers()
        keep = torch.zeros((2 * stride, 4), dtype=torch.int32, device="cuda")
        res.hits = keep.data_ptr()
        L = _lib.lib()
        for first, count in ((-1, 1), (0, 0), (2, 2), (3, 1)):
            assert L.nt_primary_hits_table_device(sc._handle, w, h, C.byref(res), stride, table._h, first, count, None, None) == _lib.NT_E_INVALID
        assert L.nt_primary_hits_table_device(sc._handle, w, h, C.byref(res), w * h - 1, table._h, 0, 1, None, None) == _lib.NT_E_INVALID
        other = render.CameraTable(n + 1, np.zeros((1, n + 1), np.float32), np.eye(n + 1, dtype=np.float32)[None])
        assert L.nt_primary_hits_table_device(sc._handle, w, h, C.byref(res), stride, other._h, 0, 1, None, None) == _lib.NT_E_INVALID


def test_the_python_device_forms_equal_the_host_form():
    """device= a torch device: tensors made by the call; out=: the caller's own tensors, written in place"""
    import torch
    case = ("feature5_n5", {})
    n, w, h = 5, 37, 21
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        host = sc.primary_hits(w, h, normals=True)
        dev = torch.device("cuda", torch.cuda.current_device())
        for device in (dev, "cuda:%d" % dev.index):
            got = sc.primary_hits(w, h, normals=True, device=device)
            assert got.item.is_cuda and tuple(got.dist.shape) == (h, w) and got.dist.dtype == torch.float32
            for key in ("dist", "item", "kind", "index", "lane", "n_transparent", "normal_origin", "normal_dir"):
                assert np.array_equal(bits(getattr(got, key).cpu().numpy()), bits(getattr(host, key))), key
        out = dict(hits=torch.full((w * h, 4), SENTINEL, dtype=torch.int32, device=dev),
                   normal_origin=torch.full((w * h, n), NSENTINEL, device=dev), normal_dir=torch.full((w * h, n), NSENTINEL, device=dev))
        got = sc.primary_hits(w, h, normals=True, out=out)
        assert got.hits is out["hits"]
        torch.cuda.synchronize()
        assert np.array_equal(out["hits"].cpu().numpy(), host.hits)
        miss = (host.item < 0).ravel()
        assert miss.any() and bool((out["normal_dir"].cpu().numpy()[miss] == NSENTINEL).all())
        assert np.array_equal(bits(out["normal_dir"].cpu().numpy()[~miss]), bits(host.normal_dir.reshape(-1, n)[~miss]))
        ri, rh = got.intersection(*np.argwhere(~miss.reshape(h, w))[0][::-1]), host.intersection(*np.argwhere(~miss.reshape(h, w))[0][::-1])
        assert ri.primitive is rh.primitive and ri.dist == rh.dist and list(ri.normal) == list(rh.normal)
        with pytest.raises(ValueError):
            sc.primary_hits(w, h, out=dict(hits=torch.zeros((w * h - 1, 4), dtype=torch.int32, device=dev)))


def test_a_larger_image_in_the_centre_first_order():
    """the 120-cell at 160 x 104: 13 tile rows and 7 quad rows, so the packet walk's quads go out through the order table"""
    case = ("cell120_n4", {})
    w, h = 160, 104
    exp = ph.expected(case, w, h)
    assert (exp["item"] >= 0).sum() >= 1000 and (exp["t0"] < 0).sum() >= 1000
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        hits, no, nd = _device_pass(sc, 4, w, h, True)
        _check(_frame(hits, no, nd, 0, w * h, w, h), exp, "cell120_n4 160x104")
        _untouched(hits, no, nd, [exp["item"]], w * h, w, h, "cell120_n4 160x104")


def _tri(nt, t, mat):
    return nt.Triangle(t["p1"], t["face_normal"], t["edge_normals"], mat)


def test_intersection_answers_with_the_objects_put_in_the_leaves():
    """the reference's known-answer scene (lib/ntracer/tests/test.py:303-363) built from Python objects, seen from the origin
    of its ray along the ray: the middle pixel is that ray"""
    ka = fx.known_answer()
    nt = NTracer(3)
    mat = Material((1, 1, 1))
    primitives = [_tri(nt, t, mat) for t in ka["triangles"]]

    def node(d):
        if d is None:
            return None
        if "leaf" in d:
            return nt.KDLeaf([primitives[i] for i in d["leaf"]])
        return nt.KDBranch(d["branch"]["axis"], d["branch"]["split"], node(d["branch"]["left"]), node(d["branch"]["right"]))

    scene = nt.CompositeScene(nt.AABB(ka["aabb"]["start"], ka["aabb"]["end"]), node(ka["tree"]))
    fwd = np.asarray(ka["ray"]["direction"], np.float64)
    right = np.cross([0.0, 1.0, 0.0], fwd)
    right /= np.linalg.norm(right)
    axes = np.asarray([right, np.cross(fwd, right), fwd], np.float32)
    origin = np.asarray(ka["ray"]["origin"], np.float32)
    fov = 0.25
    scene.set_fov(fov)
    scene._set_camera_arrays(origin, axes)
    w, h = 16, 12
    # the expected records, by the oracle on the flattened scene (triangle i of it is primitives[i])
    flat = fx.known_answer_flat(ka)
    osc = ob.OracleScene(3, origin, axes, fov)
    d = np.stack([osc.primary_dir(x, y, w, h) for y in range(h) for x in range(w)])
    t0 = ph.aabb_distance(flat["aabb_start"], flat["aabb_end"], origin, d)
    orc = rq.Oracle(3, flat, False, True)
    with pytest.MonkeyPatch.context() as mp:
        sup.set_switches(mp, ph.SWITCHES, {})
        got = scene.primary_hits(w, h, normals=True)
        seen = set()
        for y in range(h):
            for x in range(w):
                i = y * w + x
                ri = got.intersection(x, y)
                ref = None
                if t0[i] >= 0:
                    r = orc.intersects(origin[None], d[i:i + 1], t0[i:i + 1], [FLT_MAX], [-1], [-1])
                    ref = r if r["item"][0] >= 0 else None
                if ref is None:
                    assert ri is None, (x, y)
                    continue
                assert ri is not None and ri.primitive is primitives[int(ref["item"][0]) >> 2] and ri.batch_index == -1, (x, y)
                assert np.float32(ri.dist) == ref["dist"][0], (x, y)
                assert np.array_equal(np.asarray(list(ri.origin), np.float32), ref["normal_origin"][0]), (x, y)
                assert np.array_equal(np.asarray(list(ri.normal), np.float32), ref["normal"][0]), (x, y)
                seen.add(int(ref["item"][0]) >> 2)
        assert got.intersection(w // 2, h // 2).primitive is primitives[4]        # the reference's own ray
        assert len(seen) >= 2 and got.intersection(0, 0) is None
        with pytest.raises(ValueError):
            scene.primary_hits(w, h).intersection(w // 2, h // 2)                  # no normals, no RayIntersection


def test_an_empty_scene_answers_no_hit_for_every_pixel():
    g, n, flat = rq.scene("cell600_n4")
    f = dict(flat)
    f["root"] = -1
    sc = tracern.CompositeScene.from_flat(n, f)
    sc._set_camera_arrays(*ph.camera("cell600_n4"))
    got = sc.primary_hits(37, 21, normals=True)
    assert (got.item == -1).all() and (got.lane == -1).all() and (got.dist == FLT_MAX).all() and not got.n_transparent.any()
    assert not got.normal_origin.any() and not got.normal_dir.any()


def test_abort_word_raised_before_the_call_nothing_is_written():
    import torch
    for case in (("cell600_n4", {}), ("feature5_n5", {}), ("lit12_n12", {})):          # the packet walk, a per-lane walk, run-time n
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene(case, mp)
            n = rq.scene(case[0])[1]
            dev = torch.device("cuda", torch.cuda.current_device())
            w, h = 37, 21
            hits = torch.full((w * h, 4), SENTINEL, dtype=torch.int32, device=dev)
            normals = torch.full((w * h, n), NSENTINEL, dtype=torch.float32, device=dev)
            word = torch.ones(1, dtype=torch.int32, device=dev)
            res = _lib.NtHitBuffers()
            res.hits, res.normal_origin = hits.data_ptr(), normals.data_ptr()
            opts = _lib.NtRenderOpts()
            opts.device = dev.index
            opts.abort_device = word.data_ptr()
            stream = torch.cuda.current_stream(dev).cuda_stream
            assert _lib.lib().nt_primary_hits_device(sc._handle, w, h, C.byref(res), C.byref(opts), stream) == _lib.NT_OK
            torch.cuda.synchronize()
            assert bool((hits == SENTINEL).all()) and bool((normals == NSENTINEL).all()), case
