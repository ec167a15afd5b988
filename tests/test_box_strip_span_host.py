"""The span of a camera (ntracer_amd/csrc/nt_box_span.hpp, nt_box_strip_span): the interval of sx outside which no ray of the
camera can hit BoxScene's cube, which nt_camera_table_create works out once a camera and box_tile_kernel tests its column strip
against before it works out any stretch code (nt_box.hpp, NT_BOX_STRIP_SPAN).  Without a GPU:

  * soundness, on the cameras pinned here at 630 x 200 and 1920 x 1080: every pixel the oracle calls a hit has its sx inside the
    span, and every stretch whose code is 1 .. 14 lies in a strip the span keeps;
  * yield, a condition: of the 314 column strips of bench cameras 0, 8, .., 152 at 1920 x 1080 whose 1080 codes are all 0, the
    span declares at least 311 empty (and no other strip);
  * the C++ function against tools/box_sets_census.py's strip_span on every camera, the edge cameras among them: an origin
    inside the cube, on a face and at 1.0005 from the centre plane of a face (no statement), the cube behind the camera (the
    empty interval), right = 0 and up parallel to forward (no statement), one of right / up / forward 1e-4 .. 1e-30 of the others
    with the cube in full view (no statement, never the empty interval), a NaN and an infinity in the origin (no statement),
    n = 3, n = 10 and n = 11, the first dimension that goes without;
  * the probe built with -fsanitize=address,undefined on the same inputs (a stand-alone program).

cameras(n) is also what tests/test_box_strip_span_gpu.py renders."""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fixtures as fx
import oracle_binding as ob
import support as sup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import box_sets_census as census  # noqa: E402
import test_box_classify_sets as tcs  # noqa: E402
import test_box_lean_groups as tlg  # noqa: E402

F = np.float32
SIZES = ((630, 200), (1920, 1080))
DIMS = (3, 6, 8, 10)
BENCH = (0, 48, 112)             # camera 0 is axis-aligned; 48 and 112: the middle of the bench's rotation


def _direction(n):
    v = np.random.default_rng(7100 + n).standard_normal(n)
    return v / np.linalg.norm(v)


@functools.lru_cache(maxsize=None)
def _orientation(n):
    """axes of a camera on the ray through _direction(n) that looks at the centre (the same at every distance)"""
    return tcs.looking_at_centre(n, 8.0 * _direction(n), np.random.default_rng(7200 + n))[1]


def _at_distance(n, d):
    return (d * _direction(n)).astype(F), _orientation(n)


def _bisect(f, lo, hi, target):
    """d in [lo, hi] with f(d) = target, f decreasing"""
    assert f(lo) > target > f(hi), (f(lo), target, f(hi))
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if f(mid) > target:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def boundary_cameras(n, w):
    """four cameras at distances picked by bisection, so that in a w-wide frame sx_hi lies a quarter of a pixel below and above
    the first pixel of a column strip right of the middle (the strip is just skipped / just kept) and sx_lo a quarter of a pixel
    above and below the last pixel of a strip left of the middle: (name, origin, axes, strip, kept)"""
    ncols = (w + 63) // 64
    _, _, fovI = census.screen(w, 1)
    px = float(fovI)
    c_hi, c_lo = ncols // 2 + 2, ncols // 2 - 3
    first_hi, last_lo = float(census.strip_sx(w, c_hi)[0]), float(census.strip_sx(w, c_lo)[1])
    hi = lambda d: float(census.strip_span(*_at_distance(n, d))[1])
    lo = lambda d: -float(census.strip_span(*_at_distance(n, d))[0])
    out = []
    for name, f, target, strip, kept in (("hi-below", hi, first_hi - 0.25 * px, c_hi, False), ("hi-above", hi, first_hi + 0.25 * px, c_hi, True),
                                         ("lo-above", lo, -(last_lo + 0.25 * px), c_lo, False), ("lo-below", lo, -(last_lo - 0.25 * px), c_lo, True)):
        d = _bisect(f, 1.5 * np.sqrt(n) + 2.0, 200.0, target)
        o, a = _at_distance(n, d)
        out.append(("span-%s-%d" % (name, w), o, a, strip, kept))
    return out


def check_boundaries(n, w):
    """the boundary cameras do what their names say, to within half a pixel"""
    _, _, fovI = census.screen(w, 1)
    for name, o, a, strip, kept in boundary_cameras(n, w):
        lo, hi = census.strip_span(o, a)
        s0, s1 = census.strip_sx(w, strip)
        edge, bound = (float(s0), float(hi)) if "hi-" in name else (float(s1), float(lo))
        assert 0.0 < abs(bound - edge) < 0.5 * float(fovI), (name, bound, edge)
        assert bool(census.strips_kept(o, a, w)[strip]) == kept, name
        # ... and the strip beyond it is out, the strip before it in
        step = 1 if "hi-" in name else -1
        k = census.strips_kept(o, a, w)
        assert not k[strip + step] and k[strip - step], name


def inside_camera(n):
    o = np.zeros(n, F)
    o[:3] = (0.3, -0.2, 0.1)
    return o, _orientation(n)


def behind_camera(n):
    """the far camera of the boundary family, turned round: forward and right negated"""
    o, a = _at_distance(n, 9.0)
    a = np.array(a, F)
    a[0], a[2] = -a[0], -a[2]
    return o, np.ascontiguousarray(a)


@functools.lru_cache(maxsize=None)
def cameras(n):
    """(name, origin, axes): tests/test_box_lean_groups.py's (stress cameras, an origin inside the cube and on a face, diagonals, far
    and edge-on ones, at n = 6 eight of the bench's), the bench's cameras 0, 48 and 112 (n = 6), the boundary cameras of both
    widths, a camera inside the cube and one with the cube behind it"""
    cams = list(tlg.cameras(n))
    if n == 6:
        g = fx.load("box_n6_1920x1080")
        cams += [("bench-%d" % k, np.asarray(g["origins"][k], F), np.ascontiguousarray(g["axes"][k], F)) for k in BENCH if k % 20]
    for w, _ in SIZES:
        cams += [c[:3] for c in boundary_cameras(n, w)]
    cams += [("inside-cube", ) + inside_camera(n), ("cube-behind", ) + behind_camera(n)]
    return cams


def edge_cameras():
    """(name, n, origin, axes, what): what = "none", "empty" or "interval" """
    out = []
    n = 6
    out.append(("inside", n) + inside_camera(n) + ("none", ))
    rng = np.random.default_rng(7300)
    for name, x in (("on-a-face", -1.0), ("at-1.0005", -1.0005)):
        o = np.zeros(n, F)
        o[:3] = (x, 0.3, -0.25)
        out.append((name, n) + tcs.looking_at_centre(n, o, rng) + ("none", ))
    out.append(("behind", n) + behind_camera(n) + ("empty", ))
    o, a = _at_distance(n, 9.0)
    z = np.array(a, F)
    z[0] = 0.0
    out.append(("right-is-zero", n, o, z, "none"))
    z = np.array(a, F)
    z[1] = 2.0 * z[2]
    out.append(("up-along-forward", n, o, z, "none"))
    for name, bad in (("nan-origin", np.nan), ("inf-origin", np.inf)):
        z = np.array(o, F)
        z[1] = bad
        out.append((name, n, z, a, "none"))
    # one of the three axes many orders of magnitude shorter than the others: every triple's determinant is tiny and not zero,
    # the cube is in full view (with an orthonormal `up` these cameras get an interval) -- no statement, never the empty interval
    o3, f3 = np.array([-3.5, 0.0, -3.5], F), np.array([0.70710678, 0.0, 0.70710678], F)
    for name, scale in (("tiny-up-1e-13", 1e-13), ("tiny-up-1e-8", 1e-8), ("tiny-up-1e-30", 1e-30), ("tiny-up-1e-4", 1e-4)):
        up3 = np.array([-0.70710678 * scale, 0.0, 0.70710678 * scale], F)
        out.append((name, 3, o3, np.ascontiguousarray(np.stack([np.array([0.0, 1.0, 0.0], F), up3, f3])), "none"))
        o6, a6 = np.zeros(6, F), np.zeros((6, 6), F)
        o6[:3] = o3
        a6[0, 1], a6[1, :3], a6[2, :3] = 1.0, up3, f3
        out.append((name + "-6d", 6, o6, a6, "none"))
    up3 = np.array([-0.70710678, 0.0, 0.70710678], F)
    out.append(("orthonormal-up", 3, o3, np.ascontiguousarray(np.stack([np.array([0.0, 1.0, 0.0], F), up3, f3])), "interval"))
    z = np.array(a, F)
    z[0] = z[0] * F(1e-13)
    out.append(("tiny-right", n, o, z, "none"))
    z = np.array(a, F)
    z[2] = z[2] * F(1e-13)
    out.append(("tiny-forward", n, o, z, "none"))
    for m, what in ((3, "interval"), (10, "interval"), (census.SPAN_MAX_N + 1, "none")):
        out.append(("n=%d" % m, m) + _at_distance(m, 9.0) + (what, ))
    return out


def _kind(lo, hi):
    if np.isneginf(lo) and np.isposinf(hi):
        return "none"
    if lo > hi:
        return "empty"
    assert np.isfinite(lo) and np.isfinite(hi), (lo, hi)
    return "interval"


def _line(n, o, a):
    vals = np.concatenate([np.asarray(o, F), np.asarray(a, F)[0], np.asarray(a, F)[1], np.asarray(a, F)[2]])
    return "%d " % n + " ".join(repr(float(v)) for v in vals)


def _build_probe(tmp_path, extra=()):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / ("box_strip_span_probe" + ("_san" if extra else "")))
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ntracer_amd", "csrc")] + list(extra) +
                          [os.path.join(ROOT, "tests", "box_strip_span_probe.cpp"), "-o", exe])
    return exe


def _all_inputs():
    cams = [(name, n, o, a) for n in DIMS for name, o, a in cameras(n)] + [c[:4] for c in edge_cameras()]
    g = fx.load("box_n6_1920x1080")
    cams += [("bench-%d" % k, 6, np.asarray(g["origins"][k], F), np.ascontiguousarray(g["axes"][k], F)) for k in range(0, 160, 8)]
    return cams


def _run_probe(exe, cams, env=None):
    text = "\n".join(_line(n, o, a) for _, n, o, a in cams) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, env=env).stdout.split("\n")
    got = [tuple(float(v) for v in line.split()) for line in out if line.strip()]
    assert len(got) == len(cams)
    return got


def _check_against_numpy(cams, got):
    for (name, n, o, a), (clo, chi) in zip(cams, got):
        lo, hi = census.strip_span(o, a)
        assert _kind(lo, hi) == _kind(clo, chi), (name, n, lo, hi, clo, chi)
        if _kind(lo, hi) == "interval":
            assert abs(clo - float(lo)) <= 2e-6 * (1.0 + abs(clo)) and abs(chi - float(hi)) <= 2e-6 * (1.0 + abs(chi)), (name, n, lo, hi, clo, chi)


def test_the_cpp_span_is_the_numpy_span(tmp_path):
    exe = _build_probe(tmp_path)
    cams = _all_inputs()
    _check_against_numpy(cams, _run_probe(exe, cams))
    kinds = [_kind(*census.strip_span(o, a)) for _, _, o, a in cams]
    assert kinds.count("interval") >= 40 and kinds.count("none") >= 12 and kinds.count("empty") >= 5, kinds


def test_edge_cameras_get_the_statement_they_should():
    for name, n, o, a, what in edge_cameras():
        assert _kind(*census.strip_span(o, a)) == what, name
    for n in DIMS:
        assert _kind(*census.strip_span(*inside_camera(n))) == "none"
        assert _kind(*census.strip_span(*behind_camera(n))) == "empty"
        for w, _ in SIZES:
            check_boundaries(n, w)


def test_the_probe_is_clean_under_the_sanitizers(tmp_path):
    exe = _build_probe(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    cams = _all_inputs()
    _check_against_numpy(cams, _run_probe(exe, cams, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")))


def oracle_hits(n, o, a, w, h):
    """[h][w] bool: the oracle's pixel is a hit -- in fp32 channels a hit is (s, s/2, s/2) with s > 0, the background (i, i, i)
    or (0, -i, -i)"""
    img = ob.OracleScene(n, o, a).render(w, h, fx.RGBF32, threads=sup.worker_threads())
    rgb = np.ascontiguousarray(img).view(">f4").reshape(h, w, 3).astype(F)         # (the image formats are big-endian unless reversed)
    return (rgb[:, :, 0] > 0) & (rgb[:, :, 1] == rgb[:, :, 0] * F(0.5))


def sound_on(n, name, o, a, w, h):
    lo, hi = census.strip_span(o, a)
    half_w, _, fovI = census.screen(w, h)
    sx = (fovI * (np.arange(w).astype(F) - half_w)).astype(F)
    inside = (sx >= lo) & (sx <= hi)
    hits = oracle_hits(n, o, a, w, h).any(0)
    assert not (hits & ~inside).any(), (n, name, w, "the oracle hits outside the span", lo, hi, sx[hits & ~inside][:4])
    code, _ = census.stretch_codes(o, a, w, h)
    live = ((code >= 1) & (code <= 14)).any(0)
    kept = census.strips_kept(o, a, w)
    assert not (live & ~kept).any(), (n, name, w, "a stretch with a face or near-tie code in a strip the span clears", np.nonzero(live & ~kept)[0])
    return int(hits.sum()), int((~kept).sum())


@pytest.mark.parametrize("n", DIMS)
def test_no_hit_and_no_coded_stretch_lies_outside_the_span(n):
    """630 x 200: every camera; 1920 x 1080: the boundary cameras of that width, the inside and behind cameras, a far one, an
    edge-on one and (n = 6) the bench's three"""
    columns_hit = strips_out = 0
    for name, o, a in cameras(n):
        for w, h in SIZES:
            if w == 1920 and not (name.startswith(("span-", "bench-0", "bench-48", "bench-112", "inside-cube", "cube-behind")) or name in ("far-1", "edge-on-0")):
                continue
            c, s = sound_on(n, name, o, a, w, h)
            columns_hit += c
            strips_out += s
    # (the check has something to check: columns with hits, and strips the span clears)
    assert columns_hit >= 1000 and strips_out >= 50, (columns_hit, strips_out)


def test_the_span_clears_the_bench_strips_whose_codes_are_all_zero():
    g = fx.load("box_n6_1920x1080")
    zero = cleared = wrong = 0
    for k in range(0, 160, 8):
        o, a = np.asarray(g["origins"][k], F), np.ascontiguousarray(g["axes"][k], F)
        code, _ = census.stretch_codes(o, a, 1920, 1080)
        allzero = (code == 0).all(0)
        kept = census.strips_kept(o, a, 1920)
        zero += int(allzero.sum())
        cleared += int((allzero & ~kept).sum())
        wrong += int((~allzero & ~kept).sum())
    assert zero == 314, zero
    assert cleared >= 311 and wrong == 0, (cleared, wrong)
