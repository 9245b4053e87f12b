// CastRays: the first crossing of a ray with the level set {Query = iso} (include/hpsdf.h, "CastRays").  The ray is clipped to the
// root, walked leaf by leaf (the field along it is a polynomial of degree <= p inside a leaf, sampled max(1, p) times per leaf
// segment), and the first sign change of Query - iso is refined by a safeguarded Newton iteration on the directional derivative.
//
// One set of statements for the calling thread (host_query.cpp, hostCastRay) and the kernels (cast_rays.hip): the pieces -- castClip,
// castExit, castMove, castRefinePick -- and the loop that strings them together, castRay<Field>.  Field supplies the two things
// that differ between the two sides, both pinned elsewhere:
//   double eval(const double (&x)[3], double (&g)[3])   QueryGradient at a world point: the value and the world gradient, not normalised
//   void locate(const double (&pu)[3], double (&lo)[3], double (&hi)[3], int& degree)
//                                                       Query's descent of a point of the unit cube: the leaf's box (exact dyadics)
// The loop has ONE call of eval, whatever the phase (first sample, leaf samples, refinement): on the device the leaf evaluation is
// a few thousand instructions per degree class and is not to be inlined three times.
// Everything is built with -ffp-contract=off, so both sides give the same bits.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/hpsdf.h"
#include "leaf_jet.hpp"

namespace hpsdf {

struct CastArgs {
    double iso, tol;
    uint32_t maxIter;   // <= 255
    uint32_t maxCells;  // 1..65535
    uint32_t flags;     // HPSDF_CAST_UNIT
    uint32_t pad;
};

// one ray's row of outputs
struct CastRow {
    double t, x[3], f, g[3];
    uint32_t evals, cells;
    int status;
};

__host__ __device__ inline double castQuietNaN() { return __builtin_bit_cast(double, (unsigned long long)0x7FF8000000000000ull); }

// the largest double below v (v finite)
__host__ __device__ inline double castBelow(double v) {
    if (v == 0.0) return __builtin_bit_cast(double, (unsigned long long)0x8000000000000001ull);
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    return __builtin_bit_cast(double, v > 0.0 ? b - 1ull : b + 1ull);
}

__host__ __device__ inline bool castFinite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN

// step 1: a ray the walk can take
__host__ __device__ inline bool castValid(const double* o, const double* d, double tMax) {
    for (int a = 0; a < 3; ++a)
        if (!castFinite(o[a]) || !castFinite(d[a])) return false;
    if (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0) return false;
    return tMax >= 0.0;  // false for NaN
}

// step 2: the ray in the root's frame and its slabs against [-0.5, 0.5]^3; false: it misses the root within [0, tMax]
__host__ __device__ inline bool castClip(const double* o, const double* d, double tMax, const double* rootCentre, const double* rootInvSizes,
                                         double (&ou)[3], double (&du)[3], double& t0, double& t1) {
    t0 = 0.0, t1 = tMax;
    for (int a = 0; a < 3; ++a) {
        ou[a] = (o[a] - rootCentre[a]) * rootInvSizes[a];
        du[a] = d[a] * rootInvSizes[a];
    }
    for (int a = 0; a < 3; ++a) {
        if (du[a] == 0.0) {
            if (!(ou[a] >= -0.5 && ou[a] <= 0.5)) return false;
            continue;
        }
        const double tl = (-0.5 - ou[a]) / du[a];
        const double th = (0.5 - ou[a]) / du[a];
        const double tin = du[a] > 0.0 ? tl : th;
        const double tout = du[a] > 0.0 ? th : tl;
        if (tin > t0) t0 = tin;
        if (tout < t1) t1 = tout;
    }
    return t0 <= t1;
}

// the point of the unit cube the walk starts its descent from: ou + t du, each coordinate clamped into [-0.5, 0.5]
__host__ __device__ inline void castUnitPoint(const double (&ou)[3], const double (&du)[3], double t, double (&pu)[3]) {
    for (int a = 0; a < 3; ++a) {
        const double m = t * du[a];
        double p = ou[a] + m;
        if (p < -0.5) p = -0.5;
        if (p > 0.5) p = 0.5;
        pu[a] = p;
    }
}

// step 4, exit: where the ray leaves the box [lo, hi], never before t and never after t1; e: the axis of the face (-1: no axis moves)
__host__ __device__ inline double castExit(const double (&ou)[3], const double (&du)[3], const double (&lo)[3], const double (&hi)[3], double t,
                                           double t1, int& e) {
    double tb = 0.0;
    e = -1;
    for (int a = 0; a < 3; ++a) {
        if (du[a] == 0.0) continue;
        const double face = du[a] > 0.0 ? hi[a] : lo[a];
        const double ta = (face - ou[a]) / du[a];
        if (e < 0 || ta < tb) tb = ta, e = a;
    }
    if (e < 0) return t1;
    if (!(tb >= t)) tb = t;
    if (!(tb <= t1)) tb = t1;
    return tb;
}

// step 4, move across face e of [lo, hi] at parameter tb: the point the next descent starts from; false: the face is the root's own
__host__ __device__ inline bool castMove(const double (&ou)[3], const double (&du)[3], const double (&lo)[3], const double (&hi)[3], double tb,
                                         int e, double (&pu)[3]) {
    if (du[e] > 0.0) {
        if (hi[e] >= 0.5) return false;
    } else {
        if (lo[e] <= -0.5) return false;
    }
    for (int a = 0; a < 3; ++a) {
        if (a == e) {
            pu[a] = du[a] > 0.0 ? hi[a] : castBelow(lo[a]);  // the descent's >= takes the upper cell at the face itself
            continue;
        }
        const double m = tb * du[a];
        double p = ou[a] + m;
        const double top = castBelow(hi[a]);
        if (!(p >= lo[a])) p = lo[a];
        if (!(p <= top)) p = top;
        pu[a] = p;
    }
    return true;
}

// step 4, samples: sample j of S on the segment [t, tb]; the last one is tb itself
__host__ __device__ inline double castSampleT(double t, double tb, int j, int S) {
    if (j == S) return tb;
    const double w = (double)j / (double)S;
    const double m = (tb - t) * w;
    return t + m;
}

// step 5, the next point of the bracket [a, b]: Newton's from (c, rc, sc) if it lies strictly inside and the last step halved the
// bracket, else the midpoint; false: the point is not strictly inside (the bracket cannot shrink any more)
__host__ __device__ inline bool castRefinePick(double a, double b, double c, double rc, double sc, bool halved, double& m) {
    const double q = rc / sc;
    const double tn = c - q;
    if (halved && tn > a && tn < b) {
        m = tn;
    } else {
        const double w = b - a;
        m = a + 0.5 * w;
    }
    return m > a && m < b;
}

// The walk of one ray (include/hpsdf.h, "CastRays", steps 1 to 5).
template <class Field>
__host__ __device__ inline void castRay(Field& F, const double* rootCentre, const double* rootInvSizes, int leftAssoc, const double* o,
                                        const double* d, double tMax, const CastArgs& A, CastRow& R) {
    const double nan = castQuietNaN();
    R.t = nan, R.x[0] = R.x[1] = R.x[2] = nan, R.f = DBL_MAX, R.g[0] = R.g[1] = R.g[2] = nan;
    R.evals = 0, R.cells = 0;
    if (!castValid(o, d, tMax)) {
        R.status = HPSDF_CAST_INVALID;
        return;
    }
    double ou[3], du[3], t0, t1;
    if (!castClip(o, d, tMax, rootCentre, rootInvSizes, ou, du, t0, t1)) {
        R.status = HPSDF_CAST_MISS;
        return;
    }
    enum { kFirst, kSample, kRefine };
    int phase = kFirst, status = -1;
    double te = t0;                  // the parameter evaluated next
    double t = t0, tb = t0;          // the leaf segment [t, tb]
    double lo[3], hi[3], pu[3];      // the held leaf's box, the point its descent started from
    int degree = 0, e = -1, S = 1, j = 1;
    double prev = 0.0, tPrev = t0;   // the last sample that was no hit
    double ba = 0.0, bb = 0.0, ra = 0.0;               // the bracket and r at its lower end
    double fb = 0.0, gb[3] = {0.0, 0.0, 0.0};          // QueryGradient at bb
    double c = 0.0, rc = 0.0, sc = 0.0;                // the last refinement point, r and s there
    uint32_t k = 0;
    bool halved = true;
    double x[3], f, g[3];
    for (;;) {
        for (int a = 0; a < 3; ++a) {
            const double m = te * d[a];
            x[a] = o[a] + m;
        }
        f = F.eval(x, g);
        ++R.evals;
        bool walk = false, move = false;
        if (phase == kRefine) {
            if (f == DBL_MAX) {
                status = HPSDF_CAST_UNCONVERGED;
                break;
            }
            const double rm = f - A.iso;
            if (fabs(rm) <= A.tol) {
                status = HPSDF_CAST_HIT;
                break;
            }
            const double w = bb - ba;
            if ((rm < 0.0) == (ra < 0.0)) {
                ba = te, ra = rm;
            } else {
                bb = te, fb = f, gb[0] = g[0], gb[1] = g[1], gb[2] = g[2];
            }
            c = te, rc = rm, sc = sum3(g[0] * d[0], g[1] * d[1], g[2] * d[2], leftAssoc);
            halved = (bb - ba) <= 0.5 * w;
            ++k;
        } else {
            if (f == DBL_MAX) {
                status = HPSDF_CAST_MISS;
                break;
            }
            const double cur = f - A.iso;
            if (fabs(cur) <= A.tol) {
                status = HPSDF_CAST_HIT;
                break;
            }
            if (phase == kFirst) {
                prev = cur, tPrev = te;
                castUnitPoint(ou, du, t0, pu);
                F.locate(pu, lo, hi, degree);
                R.cells = 1;
                t = t0;
                walk = true;
            } else if ((prev < 0.0) != (cur < 0.0)) {
                ba = tPrev, ra = prev, bb = te, fb = f, gb[0] = g[0], gb[1] = g[1], gb[2] = g[2];
                c = te, rc = cur, sc = sum3(g[0] * d[0], g[1] * d[1], g[2] * d[2], leftAssoc);
                halved = true, k = 0;
                phase = kRefine;
            } else {
                prev = cur, tPrev = te;
                if (j < S) {
                    ++j;
                    te = castSampleT(t, tb, j, S);
                } else {
                    walk = move = true;
                }
            }
        }
        if (phase == kRefine) {
            // the row of an unconverged ray is the bracket's upper end
            if (!castRefinePick(ba, bb, c, rc, sc, halved, te) || k == A.maxIter) {
                status = HPSDF_CAST_UNCONVERGED;
                break;
            }
            continue;
        }
        if (!walk) continue;
        // the next leaf segment that has samples
        for (;;) {
            if (move) {
                if (tb >= t1 || !castMove(ou, du, lo, hi, tb, e, pu)) {
                    status = HPSDF_CAST_MISS;
                    break;
                }
                if (R.cells >= A.maxCells) {
                    status = HPSDF_CAST_CELL_LIMIT;
                    break;
                }
                F.locate(pu, lo, hi, degree);
                ++R.cells;
                t = tb;
            }
            tb = castExit(ou, du, lo, hi, t, t1, e);
            if (tb > t) {
                S = degree > 1 ? degree : 1;
                j = 1;
                te = castSampleT(t, tb, j, S);
                phase = kSample;
                break;
            }
            move = true;
        }
        if (status >= 0) break;
    }
    if (status == HPSDF_CAST_HIT) {
        R.t = te, R.x[0] = x[0], R.x[1] = x[1], R.x[2] = x[2], R.f = f, R.g[0] = g[0], R.g[1] = g[1], R.g[2] = g[2];
    } else if (status == HPSDF_CAST_UNCONVERGED) {
        R.t = bb, R.f = fb, R.g[0] = gb[0], R.g[1] = gb[1], R.g[2] = gb[2];
        for (int a = 0; a < 3; ++a) {
            const double m = bb * d[a];
            R.x[a] = o[a] + m;
        }
    }
    if ((A.flags & HPSDF_CAST_UNIT) != 0u) unitGradient(R.g, leftAssoc);
    R.status = status;
}

}  // namespace hpsdf
