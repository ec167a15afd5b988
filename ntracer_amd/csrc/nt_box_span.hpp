// The span of a camera: the one interval [sx_lo, sx_hi] of the ray source's horizontal coordinate outside which no ray of the
// camera can be a hit of BoxScene's cube, whatever its row.  Host only, plain C++ (g++ -std=c++17 -I ntracer_amd/csrc compiles
// it alone: tests/box_strip_span_probe.cpp); nt_camera_table_create works it out once a camera, and box_tile_kernel lets the
// column strips that lie outside it go around their stretch codes (nt_box.hpp, NT_BOX_STRIP_SPAN).
//
// The argument.  A ray v = fwd + right*sx - up*sy that the reference could call a hit comes within h = 1 + 2m + 1e-3 of the
// cube in every coordinate at some tau > 0 (box_stretch_code2's premise, with the same m and h, worked out in fp32 as there).
// Such (tau, a, b) = (tau, tau*sx, tau*sy) are the points with tau > 0 of the polyhedron
//     P = { -h - o_j <= tau*fwd_j + a*right_j - b*up_j <= h - o_j,  j < n },
// which is bounded when right, up and fwd are independent.  Where P lies in tau >= NT_BOX_SPAN_TAU_MIN, sx = a / tau is a
// quotient of two linear functions with a positive denominator, and its extremes over P are taken at vertices.  Every vertex
// lies on three planes of three different axes whose normals (fwd_j, right_j, -up_j) are independent, so the triples of axes,
// each with its eight choices of sides, reach them all: 8 * C(n, 3) solves of a 3 x 3 system, 960 at n = 10.
//
// The arithmetic is double, and NO triple that could hold a vertex is ever passed over.  The axes are taken in order, and an
// axis that forms, with two axes already taken, a triple whose determinant is not zero but below 1e-6 of the product of its
// normals' lengths -- two axes with nearly the same normal, as a camera turned in the plane of two coordinates has in all the
// others; or one of right / up / fwd many orders of magnitude shorter than the others, which makes EVERY triple such a one --
// would give a vertex to fewer digits than the feasibility test assumes: that axis is LEFT OUT, constraint and all.  Fewer
// constraints make P larger and the interval wider, never narrower (and of two planes that nearly coincide the second adds
// next to nothing).  Among the axes kept every triple then either has a determinant of at least 1e-6 and is solved, or one that
// is zero as computed (a zero normal; planes that are parallel to the last bit, whose common points, if any, lie on other
// triples as well).  What is kept must still span three dimensions, with right, up and fwd of comparable length (each squared
// length at least 1e-6 of the largest: the Gram test alone does not see the scale of a column) and a Gram determinant above
// 1e-6 of the product of the squared lengths; otherwise there is no statement.  A vertex counts when it
// satisfies every constraint kept to 1e-7 of (h + max |o_j|): too many vertices only widen the result.  The interval is then
// widened by NT_BOX_SPAN_SLACK * (1 + |sx|) on either side -- a sixth of a pixel of a 1920-wide frame, a thousand times the
// rounding of the fp32 direction that the kernel's own cull allows 1e-6 for -- and rounded outwards to fp32.
//
// No statement, (-inf, +inf): P reaches tau <= NT_BOX_SPAN_TAU_MIN (the origin in, on or next to the grown cube: box_color's
// business), an input that is not finite, right / up / fwd not independent or of lengths 1000 : 1 apart, n < 3 or n > NT_BOX_SPAN_MAX_N (vertex enumeration
// grows with n^3 and the dimensions beyond ten go without, as they go without tie sets).
// The empty interval, (+inf, -inf): P has no point with tau > 0 -- the cube lies behind the camera, or the camera's
// three-space misses the grown cube altogether: every pixel is background.
#pragma once
#include <cmath>
#include <limits>

#ifndef NT_BOX_SPAN_MAX_N
#define NT_BOX_SPAN_MAX_N 10
#endif
#define NT_BOX_SPAN_SLACK 1e-4
#define NT_BOX_SPAN_TAU_MIN 1e-3
// m of box_classify / box_resolve / box_cull_kernel / box_stretch_code2, per unit of 1 + max|o_j| (nt_box.hpp says what it has to
// dominate).  THE definition: nt_box.hpp and nt_var.hip get it from here.
#ifndef NT_BOX_MARGIN
#define NT_BOX_MARGIN 1e-5f
#endif

struct NtBoxSpan { float lo, hi; };

static inline NtBoxSpan nt_box_strip_span(int n, const float *origin, const float *right, const float *up, const float *fwd) {
    const float inf = std::numeric_limits<float>::infinity();
    const NtBoxSpan none = {-inf, inf}, empty = {inf, -inf};
    if (n < 3 || n > NT_BOX_SPAN_MAX_N || !origin || !right || !up || !fwd) return none;
    float omax = 0.0f;
    for (int j = 0; j < n; ++j) {
        if (!std::isfinite(origin[j]) || !std::isfinite(right[j]) || !std::isfinite(up[j]) || !std::isfinite(fwd[j])) return none;
        omax = std::fmax(omax, std::fabs(origin[j]));
    }
    // m and h as box_stretch_code2 rounds them
    const float mf = NT_BOX_MARGIN * (1.0f + omax);
    const float hf = 1.0f + 2.0f * mf + 1e-3f;
    const double h = (double)hf;
    // plane j: c_j . (tau, a, b) in [L_j, U_j]
    double c[NT_BOX_SPAN_MAX_N][3], L[NT_BOX_SPAN_MAX_N], U[NT_BOX_SPAN_MAX_N], len[NT_BOX_SPAN_MAX_N];
    for (int j = 0; j < n; ++j) {
        c[j][0] = (double)fwd[j];
        c[j][1] = (double)right[j];
        c[j][2] = -(double)up[j];
        L[j] = -h - (double)origin[j];
        U[j] = h - (double)origin[j];
        len[j] = std::sqrt(c[j][0] * c[j][0] + c[j][1] * c[j][1] + c[j][2] * c[j][2]);
    }
    auto det3 = [&](int i, int j, int k) {
        return c[i][0] * (c[j][1] * c[k][2] - c[j][2] * c[k][1]) - c[i][1] * (c[j][0] * c[k][2] - c[j][2] * c[k][0]) + c[i][2] * (c[j][0] * c[k][1] - c[j][1] * c[k][0]);
    };
    // the axes kept (see above): ks[0 .. nk)
    int ks[NT_BOX_SPAN_MAX_N], nk = 0;
    for (int q = 0; q < n; ++q) {
        bool doubtful = false;
        for (int a = 0; a < nk && !doubtful; ++a)
            for (int b = a + 1; b < nk && !doubtful; ++b) {
                const double rel = std::fabs(det3(ks[a], ks[b], q)) / (len[ks[a]] * len[ks[b]] * len[q]);
                doubtful = rel > 0.0 && rel < 1e-6;              // (a zero length: NaN, not doubtful)
            }
        if (!doubtful) ks[nk++] = q;
    }
    // independence: the Gram determinant (the squared volume the three vectors span, over the axes kept) against the product of
    // their squared lengths
    double gram[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int a = 0; a < nk; ++a)
        for (int p = 0; p < 3; ++p)
            for (int q = 0; q < 3; ++q) gram[p][q] += c[ks[a]][p] * c[ks[a]][q];
    const double gdet = gram[0][0] * (gram[1][1] * gram[2][2] - gram[1][2] * gram[2][1]) - gram[0][1] * (gram[1][0] * gram[2][2] - gram[1][2] * gram[2][0]) +
                        gram[0][2] * (gram[1][0] * gram[2][1] - gram[1][1] * gram[2][0]);
    const double gscale = gram[0][0] * gram[1][1] * gram[2][2];
    const double gmax = std::fmax(gram[0][0], std::fmax(gram[1][1], gram[2][2])), gmin = std::fmin(gram[0][0], std::fmin(gram[1][1], gram[2][2]));
    if (!(gscale > 0.0) || !(gmin >= 1e-6 * gmax) || !(gdet > 1e-6 * gscale)) return none;
    const double tol = 1e-7 * (h + (double)omax);
    double tau_min = INFINITY, tau_max = -INFINITY, lo = INFINITY, hi = -INFINITY;
    int nverts = 0;
    for (int ai = 0; ai < nk; ++ai)
        for (int aj = ai + 1; aj < nk; ++aj) {
            const int i = ks[ai], j = ks[aj];
            // (c_i x c_j: shared by the third axes)
            const double x0 = c[i][1] * c[j][2] - c[i][2] * c[j][1], x1 = c[i][2] * c[j][0] - c[i][0] * c[j][2], x2 = c[i][0] * c[j][1] - c[i][1] * c[j][0];
            for (int ak = aj + 1; ak < nk; ++ak) {
                const int k = ks[ak];
                const double det = x0 * c[k][0] + x1 * c[k][1] + x2 * c[k][2];
                const double rel = std::fabs(det) / (len[i] * len[j] * len[k]);
                // (among the axes kept det3 found at least 1e-6, or zero -- here, in another order of operations, zero up to
                // rounding -- or NaN from a zero length)
                if (!(rel >= 1e-9)) continue;
                // the inverse's rows of cofactors: p = (d_i (c_j x c_k) + d_j (c_k x c_i) + d_k (c_i x c_j)) / det
                const double y0 = c[j][1] * c[k][2] - c[j][2] * c[k][1], y1 = c[j][2] * c[k][0] - c[j][0] * c[k][2], y2 = c[j][0] * c[k][1] - c[j][1] * c[k][0];
                const double z0 = c[k][1] * c[i][2] - c[k][2] * c[i][1], z1 = c[k][2] * c[i][0] - c[k][0] * c[i][2], z2 = c[k][0] * c[i][1] - c[k][1] * c[i][0];
                const double inv = 1.0 / det;
                for (int s = 0; s < 8; ++s) {
                    const double di = (s & 1) ? U[i] : L[i], dj = (s & 2) ? U[j] : L[j], dk = (s & 4) ? U[k] : L[k];
                    const double tau = (di * y0 + dj * z0 + dk * x0) * inv, a = (di * y1 + dj * z1 + dk * x1) * inv, b = (di * y2 + dj * z2 + dk * x2) * inv;
                    bool inside = true;
                    for (int aq = 0; aq < nk && inside; ++aq) {
                        const int q = ks[aq];
                        if (q == i || q == j || q == k) continue;
                        const double v = c[q][0] * tau + c[q][1] * a + c[q][2] * b;
                        inside = v >= L[q] - tol && v <= U[q] + tol;
                    }
                    if (!inside) continue;
                    ++nverts;
                    tau_min = std::fmin(tau_min, tau);
                    tau_max = std::fmax(tau_max, tau);
                    if (tau > 0.0) {
                        const double sx = a / tau;
                        lo = std::fmin(lo, sx);
                        hi = std::fmax(hi, sx);
                    }
                }
            }
        }
    if (nverts == 0 || tau_max <= -NT_BOX_SPAN_TAU_MIN) return empty;
    if (!(tau_min > NT_BOX_SPAN_TAU_MIN) || !std::isfinite(lo) || !std::isfinite(hi)) return none;
    lo -= NT_BOX_SPAN_SLACK * (1.0 + std::fabs(lo));
    hi += NT_BOX_SPAN_SLACK * (1.0 + std::fabs(hi));
    NtBoxSpan r;
    r.lo = (float)lo;
    if ((double)r.lo > lo) r.lo = std::nextafterf(r.lo, -inf);
    r.hi = (float)hi;
    if ((double)r.hi < hi) r.hi = std::nextafterf(r.hi, inf);
    return r;
}
