"""The Solid family on the device: the torture scenes of tests/solid_cases.py -- 40 Solids and no simplex, nested and coincident
Solids, two mirrors, Solids poking through batches -- at every fixed N and at run-time n = 11, 17, 33, 64, from outside and from
inside a sphere and a cube, against the oracle bit for bit (dist, item, lane, normal rays, colours) and, outside the margin,
against the float64 brute force (which primitive, dist within solid_cases.TOLERANCE).  The kernel every call lands on is
solid_cases.route's; tests/test_solids_host.py holds the table of them against the sources, without a GPU.

Each test runs its GPU work once; nothing is retried."""
import numpy as np
import pytest

import fixtures as fx
import ntracer_amd
import solid_cases as sc
import support as sup
from ntracer_amd import _lib, tracern

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = sc.VIEW
PAD, SENTINEL = 36, 0xA7


def _id(case):
    return "%s-n%d" % case


def _label(name, n, kind, env, cam=None):
    return "%s n=%d %s %s%s" % (name, n, kind, ",".join("%s=%s" % (k[len("NTRACER_"):], v) for k, v in sorted(env.items())) or "default",
                                "" if cam is None else " camera %d" % cam)


def _scene(name, n, kind, env, mp, cam=0):
    """the scene with the switches set before it is made"""
    sup.set_switches(mp, sc.SWITCHES, env)
    s = tracern.CompositeScene.from_flat(n, sc.scene_flat(name, n, "transparent" if kind == "default" else kind))
    if kind not in ("default", "opaque"):
        s.set_params_flat(sc.params(name, n, kind))
    o, a = sc.cameras(name, n)[cam]
    s._set_camera_arrays(o, a)
    return s


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _render(s, w=W, h=H):
    """one RGBF32 frame into a padded, sentinel-filled host buffer: (the pixels' bytes (h, w * 12), padding bytes written)"""
    fmt = ntracer_amd.ImageFormat(w, h, [ntracer_amd.Channel(*c) for c in fx.RGBF32], w * 12 + PAD)
    buf = bytearray([SENTINEL]) * (fmt.pitch * h)
    assert ntracer_amd.BlockingRenderer().render(buf, fmt, s)
    a = np.frombuffer(bytes(buf), np.uint8).reshape(h, fmt.pitch)
    return a[:, :w * 12].copy(), int((a[:, w * 12:] != SENTINEL).sum())


def _same_colours(got, want, label):
    """fp32 colours bit for bit; the largest difference is printed before anything is asserted"""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    if len(bad):
        print("%s: %d floats differ from the oracle, largest difference %g" % (label, len(bad), float(np.abs(got.astype(np.float64) - want).max())))
    assert len(bad) == 0, "%s: %d floats differ from the oracle (largest difference %g), first at %r: got %r, oracle %r" % (
        label, len(bad), float(np.abs(got.astype(np.float64) - want).max()), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ------------------------------------------------------------------ queries
def _check_intersect(got, ref, label):
    item = np.where(got["kind"] < 0, -1, (got["index"] << 2) | got["kind"])
    for k, g in (("item", item), ("lane", got["lane"]), ("n_transparent", got["n_transparent"])):
        bad = np.nonzero(g != ref[k])[0]
        assert len(bad) == 0, "%s: %s differs on %d rays, first %d: got %r, oracle %r" % (label, k, len(bad), bad[0], g[bad[0]], ref[k][bad[0]])
    bad = np.nonzero(bits(got["dist"]) != bits(ref["dist"]))[0]
    assert len(bad) == 0, "%s: dist differs on %d rays, first %d: got %r, oracle %r" % (label, len(bad), bad[0], got["dist"][bad[0]], ref["dist"][bad[0]])
    hit = item >= 0
    for k in ("normal_origin", "normal"):
        bad = np.nonzero((bits(got[k][hit]) != bits(ref[k][hit])).any(axis=1))[0]
        assert len(bad) == 0, "%s: %s differs on %d rays with a hit, first %d (largest difference %g)" % (
            label, k, len(bad), np.nonzero(hit)[0][bad[0]], float(np.abs(got[k][hit].astype(np.float64) - ref[k][hit]).max()))
        assert not got[k][~hit].any(), "%s: %s written for a ray without an opaque hit" % (label, k)
    return item


@pytest.mark.parametrize("case", sc.scene_dims(), ids=_id)
def test_queries_equal_the_oracle_and_agree_with_float64(case):
    """intersect_rays with normals and occludes_rays on every batch, in both normal modes (and under NTRACER_FORCE_VAR where
    solid_cases.FORCED_VAR says so); KDNode.intersects / occludes on a sample of each batch agree with the batched forms"""
    name, n = case
    for variant, env in sc.query_cases(name, n):
        b = sc.batches(name, n, variant)
        clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
        label = _label(name, n, variant, env)
        with pytest.MonkeyPatch.context() as mp:
            s = _scene(name, n, variant, env, mp)
            args = (b.i_origins, b.i_directions, b.i_t_near, b.i_t_far, b.i_skip_item, b.i_skip_lane)
            got = s.intersect_rays(*args, normals=True)
            item = _check_intersect(got, b.i_ref[clean], label + " intersects")
            worst = sc.compare_with_float64(b, dict(dist=got["dist"], item=item), label + " intersects")
            occ = s.occludes_rays(b.o_origins, b.o_directions, b.o_distance, b.i_t_near, b.i_t_far, b.i_skip_item, b.i_skip_lane)
            for k in ("blocked", "n_transparent"):
                bad = np.nonzero(np.asarray(occ[k]) != b.o_ref[k])[0]
                assert len(bad) == 0, "%s occludes: %s differs on %d rays, first %d" % (label, k, len(bad), bad[0])
            if not env and variant == "default":
                # ---- one ray at a time through the tree's root: the first two rays of every batch and its last one
                root = s.root
                for key, sl in b.slices.items():
                    for i in sorted({sl.start, min(sl.start + 1, sl.stop - 1), sl.stop - 1}):
                        source = s._object_of(int(b.i_skip_item[i]) & 3, int(b.i_skip_item[i]) >> 2) if b.i_skip_item[i] >= 0 else None
                        hits = root.intersects(b.i_origins[i], b.i_directions[i], source=source)
                        assert len(hits) - (1 if got["kind"][i] >= 0 else 0) == min(int(got["n_transparent"][i]), _lib.NT_TH_MAX), (label, key, i)
                        if got["kind"][i] >= 0:
                            h = hits[-1]
                            assert f32(h.dist) == got["dist"][i] and h.primitive is s._object_of(int(got["kind"][i]), int(got["index"][i])), (label, key, i)
                            assert np.array_equal(np.asarray(list(h.normal), f32), got["normal"][i]), (label, key, i)
                        blocked, through = root.occludes(b.o_origins[i], b.o_directions[i], float(b.o_distance[i]), source=source)
                        assert blocked == bool(occ["blocked"][i]) and (blocked or len(through) == min(int(occ["n_transparent"][i]), _lib.NT_TH_MAX)), (label, key, i)
            assert not s.locked
        print("%s: %d rays equal the oracle bit for bit; against float64 dist within %g relative, nearer than %g within %g ulps" % (
            label, len(b.i_origins), worst[0], sc.NEAR, worst[1]))


# ------------------------------------------------------------------ renders and probes
@pytest.mark.parametrize("case", sc.scene_dims(), ids=_id)
def test_renders_probes_and_ray_colours_equal_the_oracle(case):
    """render (97 x 61 RGBF32), colors_at on a lattice and ray_colors of the lattice's own rays, for every case of
    solid_cases.render_cases: every parameter set in both normal modes, the cameras inside a sphere and inside a cube, the switches
    that change the route, and NTRACER_FORCE_VAR where FORCED_VAR says so"""
    name, n = case
    xs, ys = sc.lattice()
    failures = []
    for kind, env, cam in sc.render_cases(name, n):
        clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
        label = _label(name, n, kind, env, cam)
        with pytest.MonkeyPatch.context() as mp:
            s = _scene(name, n, kind, env, mp, cam)
            img, stray = _render(s)
            probes = s.colors_at(xs, ys, W, H)
            o, d, want_rays = sc.ray_colours(name, n, kind, cam, clean)
            rays = s.ray_colors(o, d)
        assert stray == 0, "%s: %d bytes of pitch padding written" % (label, stray)
        for what, got, want in (("render", img.view(">f4").astype(f32), sc.frame(name, n, kind, cam, clean)),
                                ("colors_at", probes, sc.probes(name, n, kind, cam, clean)), ("ray_colors", rays, want_rays)):
            try:
                _same_colours(got, want, label + " " + what)
            except AssertionError as e:
                failures.append(str(e))
        # the frame is not background alone, nor one colour
        fr = sc.frame(name, n, kind, cam, clean).reshape(H, W, 3)
        assert cam != 0 or len(np.unique(fr.reshape(-1, 3), axis=0)) >= 50, label
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ primary hits
def _check_hits(hits, rec, bf, name, n, label):
    got = dict(dist=hits.dist, item=hits.item, lane=hits.lane, n_transparent=hits.n_transparent)
    for key in ("item", "lane", "n_transparent"):
        bad = np.argwhere(np.asarray(got[key]) != rec[key])
        assert len(bad) == 0, "%s: %s differs on %d pixels, first (y, x) = %r: got %r, oracle %r" % (
            label, key, len(bad), tuple(bad[0]), got[key][tuple(bad[0])], rec[key][tuple(bad[0])])
    assert np.array_equal(bits(got["dist"]), bits(rec["dist"])), "%s: dist differs on %d pixels" % (label, int((bits(got["dist"]) != bits(rec["dist"])).sum()))
    hit = rec["item"] >= 0
    for key, rkey in (("normal_origin", "normal_origin"), ("normal_dir", "normal")):
        g = np.asarray(getattr(hits, key))
        assert np.array_equal(bits(g[hit]), bits(rec[rkey][hit])), "%s: %s differs on pixels with a hit, largest difference %g" % (
            label, key, float(np.abs(g[hit].astype(np.float64) - rec[rkey][hit]).max()))
    # ---- float64: the primitive under every pixel outside the margin, and its depth
    safe = bf.safe.reshape(hit.shape)
    assert (~safe).sum() <= sc.CAP * safe.size, (label, int((~safe).sum()))
    gi, wi = sc.canonical(name, got["item"]), sc.canonical(name, bf.item.reshape(hit.shape))
    bad = np.argwhere(safe & (gi != wi))
    assert len(bad) == 0, "%s: float64 names another primitive on %d pixels, first (y, x) = %r: got %d, float64 %d" % (
        label, len(bad), tuple(bad[0]), gi[tuple(bad[0])], wi[tuple(bad[0])])
    both = safe & (wi >= 0)
    want = bf.dist.reshape(hit.shape)[both]
    worst = float((np.abs(got["dist"][both].astype(np.float64) - want) / want).max()) if both.any() else 0.0
    assert worst <= sc.TOLERANCE[n][0], "%s: depth differs from float64 by %g relative (allowed %g)" % (label, worst, sc.TOLERANCE[n][0])
    return worst


@pytest.mark.parametrize("case", sc.scene_dims(), ids=_id)
def test_primary_hits_equal_the_oracle_and_agree_with_float64(case):
    """depth, item, lane and the normal rays of the three cameras' views equal the oracle's; the primitive id and the depth agree
    with float64 outside the margin -- from inside a sphere or a cube as from outside"""
    name, n = case
    w, h = sc.QUERY_VIEW
    for kind, env, cam in sc.hits_cases(name, n):
        clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
        label = _label(name, n, kind, env, cam) + " primary hits"
        rec, bf = sc.hit_records(name, n, kind, cam, clean)
        with pytest.MonkeyPatch.context() as mp:
            s = _scene(name, n, kind, env, mp, cam)
            hits = s.primary_hits(w, h, normals=True)
        worst = _check_hits(hits, rec, bf, name, n, label)
        if cam == 0:
            assert (rec["item"] >= 0).sum() >= 90, label
    print("%s n=%d: primary hits equal the oracle bit for bit, depth within %g of float64" % (name, n, worst))


@pytest.mark.parametrize("n", (5, 17))
def test_a_solid_is_invisible_from_inside(n):
    """the opaque field from the camera inside a sphere: no pixel's primitive is the enclosing sphere -- the reference finds the
    near root of the quadratic alone, and that is behind the camera -- and the pixels name what stands behind it, float64's
    primitive on every pixel outside the margin, a hundred of them and more; from the camera inside a cube likewise"""
    w, h = sc.QUERY_VIEW
    for cam, inside in ((1, sc.INSIDE_SPHERE["field"]), (2, sc.INSIDE_CUBE["field"])):
        rec, bf = sc.hit_records("field", n, "unlit", cam, False)
        with pytest.MonkeyPatch.context() as mp:
            s = _scene("field", n, "unlit", {}, mp, cam)
            hits = s.primary_hits(w, h)
        item = np.asarray(hits.item)
        assert (item != ((inside << 2) | _lib.KIND_SOLID)).all(), (n, cam)
        safe = bf.safe.reshape(h, w)
        want = bf.item.reshape(h, w)
        assert np.array_equal(item[safe], want[safe]), (n, cam, int((item != want)[safe].sum()))
        assert (want[safe] >= 0).sum() >= 100, (n, cam, int((want[safe] >= 0).sum()))


# ------------------------------------------------------------------ the two projections
@pytest.mark.parametrize("n", sc.PROJECTION_DIMS)
def test_field_under_a_fisheye_lens_and_the_parallel_projection(n):
    """one render of field per projection and case of solid_cases.projection_cases -- the packet walks of nt_lens.hpp and
    nt_parallel.hpp in their forms with unbatched primitives, and the ray route behind lens_expand / parallel_expand -- against
    the oracle's colours of the same rays (lens_cases and parallel_cases make the rays)"""
    import lens_cases as lc
    import parallel_cases as pc
    import ray_color_cases as rc
    w, h = sc.PROJECTION_VIEW
    origin, axes = sc.cameras("field", n)[0]
    lens = lc.LENSES["fisheye"](w, h)
    live = ~lens.masked.reshape(-1)
    v = lens.directions(lc.camera_of(origin, axes))
    org, fwd = pc.parallel_rays(origin, axes, w, h, sc.PARALLEL_HALF_WIDTH)
    failures = []
    for kind, env in sc.projection_cases(n):
        clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
        colour = rc.CentrePixel(n, sc.scene_flat("field", n, kind), sc.params("field", n, kind), clean, False)
        want_lens = np.zeros((w * h, 3), f32)
        want_lens[live] = colour.colors(origin, v[live])
        want_par = colour.colors(org, np.repeat(fwd[None], len(org), axis=0))
        assert len(np.unique(want_lens[live], axis=0)) >= 50 and len(np.unique(want_par, axis=0)) >= 50
        label = _label("field", n, kind, env)
        with pytest.MonkeyPatch.context() as mp:
            s = _scene("field", n, kind, env, mp)
            s.set_lens(lens)
            got_lens, stray = _render(s, w, h)
            s.set_lens(None)
            s.set_parallel_projection(sc.PARALLEL_HALF_WIDTH)
            got_par, stray2 = _render(s, w, h)
            s.set_parallel_projection(None)
        assert stray == 0 and stray2 == 0, label
        for what, got, want in (("fisheye", got_lens, want_lens), ("parallel", got_par, want_par)):
            # (an fp32 format clamps to 0 .. 1; + 0.0: the clamp gives +0 where the oracle's colour is -0)
            want = (np.clip(want, 0.0, 1.0) + 0.0).astype(f32)
            try:
                _same_colours(got.view(">f4").astype(f32).reshape(w * h, 3), want, "%s %s" % (label, what))
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "\n".join(failures)


def test_clip_planes_are_refused_for_every_scene():
    """NT_E_UNSUPPORTED, before a device is touched: the check of tests/test_solids_host.py, on this machine too"""
    from test_solids_host import test_clip_planes_are_refused_for_every_scene_before_a_device_is_touched as check
    check()
