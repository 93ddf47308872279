// nw_poisson_core.h -- the definition of the screened Poisson grid solver (include/nw_poisson.h), free of HIP: what a sample adds to a
// level's integer sums, the depth rule, a node's row of the linear system, one red-black update, the residual, the prolongation and the
// quantisation of the solution into the uint64 field the surface nets take.  csrc/nw_poisson.hip runs these functions one node or one
// sample a lane; tests/test_poisson_core_cpu.py compiles them with g++ and asks for the bits of tests/screened_poisson_ref.py.
// Nothing may be contracted into an fma: compile with -ffp-contract=off.  Without a HIP compiler NWO_HD is plain `inline`.
//
// This is NOT Kazhdan's (pymeshlab's) octree solver: it is a complete cube of 2^depth nodes an axis with piecewise-linear splats and a
// cascadic coarse-to-fine Gauss-Seidel solve.  The definition is this project's own:
//
//   samples     (n,3) float32 positions and outward normals.  unit = n / sqrt((nx nx + ny ny) + nz nz) in float64; a length of 0 is not
//               used (and counted).  use_lengths takes the normal as given and refuses a component above 1 in magnitude.
//               nq = rint(unit 2^12) per axis, |nq| <= 2^12.  At most NWO_MAX_N = 2^25 samples.
//   lattice     lo[3], h (float32), 3 <= depth <= 9.  Level l has n_l = 2^l nodes an axis, node i at lo + (i + 1/2) h_l,
//               h_l = (double)h 2^(depth - l): cell-centred, as the surface nets place nodes.  The base level is 2.
//   splat       per axis u = ((double)p - (double)lo) / h_l - 0.5, i0 = floor(u), q = rint((u - i0) 128), 0 <= q <= 128: weight 128 - q on
//               node i0 and q on i0 + 1, both indices clamped into [0, n_l - 1] (in float64, before any conversion: a sample far outside
//               the cube lands on the border nodes).  A sample adds w = wx wy wz to W and w nq_a to V_a at its eight nodes.
//               Proof that nothing overflows.  The eight w add up to 128^3 = 2^21, so sum W = N 2^21 <= 2^46 and a node's
//               |V_a| <= 2^21 2^12 2^25 = 2^58 < 2^63.  The sums are integers: exact, and independent of any order.
//   occupancy   a sample's home node is clamp(floor(u + 0.5)) per axis; occ_l counts the distinct home nodes of level l.
//   depth used  used = 2; for l = 3 .. depth: stop if l > max(fulldepth, 2) and (double)N_used < samplespernode (double)occ_l; else
//               used = l.  One global rule: the solve ends and the surface is extracted at `used`, h_used = h 2^(depth - used).
//   system      at level l with s = 2^(used - l): What = (double)W / 2^21, Vhat_a = -(double)V_a / 2^33 (the target gradient is the
//               inward normal: chi is high inside).  For the edge c -> c + e_a: g = 0.5 (Vhat_a[c] + Vhat_a[c + e_a]).  rhs[c] starts at
//               0 and takes, in the axis order x y z, + g of the edge below c, then - g of the edge above c (edges that leave the lattice
//               do not exist); then rhs *= 1 / s^2.  diag[c] = deg[c] + (alpha / s) What[c], deg = the in-lattice neighbours (3 .. 6).
//               alpha = (pointweight occ_used) / N_used in float64, pointweight > 0.  These are the normal equations of
//               sum over edges (chi_b - chi_a - g)^2 + (alpha / s) sum What chi^2 with free (Neumann) faces.
//   relaxation  red-black sweeps, colour (i + j + k) & 1, even first, in place: chi[c] = (rhs[c] + S) / diag[c], S = 0 plus the present
//               neighbours in the order -x +x -y +y -z +z.  A node reads the other colour only: the result does not depend on the launch.
//   residual    max over c of |rhs - (diag chi - S)|: a maximum, so free of any order.
//   prolongation axis by axis, x then y then z: out[2 I + b] = 0.75 a[I] + 0.25 a[I + (b ? 1 : -1)], the neighbour clamped at the border.
//   field       M = max |chi|, E = the smallest power of two >= M, F = (uint64)(rint(chi / E 2^31) + 2^31), 0 <= F <= 2^32.
//               thr = floor(sum W F / sum W), the mean of the interpolated chi over the samples (Kazhdan's iso-value), from the two 16-bit
//               limbs of F.  Proof.  F = Fh 2^16 + Fl with Fl < 2^16 and Fh <= 2^16; sum W Fl < 2^46 2^16 = 2^62 and
//               sum W Fh <= 2^62: 64-bit sums suffice, and the division is done in 128 bits on the host.
#ifndef NW_POISSON_CORE_H_
#define NW_POISSON_CORE_H_

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define NWO_HD __host__ __device__ __forceinline__
#else
#define NWO_HD inline
#endif

#define NWO_MAX_N (1ll << 25)
#define NWO_NORMAL_BITS 12
#define NWO_WEIGHT_BITS 7
#define NWO_FIELD_BITS 31
#define NWO_BASE_LEVEL 2
#define NWO_MIN_DEPTH 3
#define NWO_MAX_DEPTH 9
#define NWO_W_ONE 2097152.0            /* 2^21 = 2^(3 NWO_WEIGHT_BITS) */
#define NWO_V_ONE 8589934592.0         /* 2^33 = 2^(3 NWO_WEIGHT_BITS + NWO_NORMAL_BITS) */
#define NWO_F_HALF 2147483648.0        /* 2^31 */

// ---- samples ------------------------------------------------------------------------------------------------------------------------------
// nq[3] of one normal -> 1: used; 0: its length is 0, not used; -1: use_lengths and a component above 1 in magnitude.  The input is finite.
NWO_HD int nwo_normal(float fx, float fy, float fz, int use_lengths, int *nq)
{
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    const double len = sqrt((x * x + y * y) + z * z);
    nq[0] = nq[1] = nq[2] = 0;
    if (use_lengths && (fabs(x) > 1.0 || fabs(y) > 1.0 || fabs(z) > 1.0)) return -1;
    if (!(len > 0.0)) return 0;
    const double one = (double)(1 << NWO_NORMAL_BITS);
    if (use_lengths) {
        nq[0] = (int)rint(x * one); nq[1] = (int)rint(y * one); nq[2] = (int)rint(z * one);
    } else {
        nq[0] = (int)rint((x / len) * one); nq[1] = (int)rint((y / len) * one); nq[2] = (int)rint((z / len) * one);
    }
    return 1;
}

NWO_HD double nwo_spacing(float h, int depth, int level) { return (double)h * (double)(1 << (depth - level)); }

NWO_HD double nwo_u(float p, float lo, double hl) { return ((double)p - (double)lo) / hl - 0.5; }

NWO_HD int nwo_clamp_node(double i, int n) { return (int)fmin(fmax(i, 0.0), (double)(n - 1)); }

// the two nodes of one coordinate and the weight q of the upper one (the lower one has 128 - q)
NWO_HD void nwo_axis(float p, float lo, double hl, int n, int *ia, int *ib, int *q)
{
    const double u = nwo_u(p, lo, hl);
    const double fl = floor(u);
    *q = (int)rint((u - fl) * (double)(1 << NWO_WEIGHT_BITS));
    *ia = nwo_clamp_node(fl, n);
    *ib = nwo_clamp_node(fl + 1.0, n);
}

NWO_HD int nwo_home(float p, float lo, double hl, int n) { return nwo_clamp_node(floor(nwo_u(p, lo, hl) + 0.5), n); }

// node (i, j, k) of a level of 2^level nodes an axis, x fastest
NWO_HD int64_t nwo_lin(int level, int i, int j, int k) { return ((((int64_t)k << level) | (int64_t)j) << level) | (int64_t)i; }

// ---- the depth rule and the screen's weight (host) ----------------------------------------------------------------------------------------
NWO_HD int nwo_depth_used(int64_t n_used, const int64_t *occ /* [depth + 1], by level */, int depth, int fulldepth, double samples_per_node)
{
    int used = NWO_BASE_LEVEL;
    const int full = fulldepth > NWO_BASE_LEVEL ? fulldepth : NWO_BASE_LEVEL;
    for (int l = NWO_BASE_LEVEL + 1; l <= depth; ++l) {
        if (l > full && (double)n_used < samples_per_node * (double)occ[l]) break;
        used = l;
    }
    return used;
}

NWO_HD double nwo_alpha(double pointweight, int64_t occ_used, int64_t n_used) { return (pointweight * (double)occ_used) / (double)n_used; }

// ---- the system of a level ----------------------------------------------------------------------------------------------------------------
NWO_HD double nwo_vhat(long long v) { return -(double)v / NWO_V_ONE; }

// W: n^3 int64; V: the three planes of n^3 int64 one after the other.  alpha_s = alpha / s, inv_s2 = 1 / s^2
NWO_HD void nwo_system_node(const long long *W, const long long *V, int level, int i, int j, int k, double alpha_s, double inv_s2, double *rhs,
                            double *diag)
{
    const int n = 1 << level;
    const int64_t c = nwo_lin(level, i, j, k), plane = (int64_t)1 << (3 * level);
    const int at[3] = {i, j, k};
    double r = 0.0, deg = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 0; a < 3; ++a) {
        const long long *Va = V + a * plane;
        const int64_t step = (int64_t)1 << (a * level);
        const double here = nwo_vhat(Va[c]);
        if (at[a] > 0) { r += 0.5 * (nwo_vhat(Va[c - step]) + here); deg += 1.0; }
        if (at[a] < n - 1) { r -= 0.5 * (here + nwo_vhat(Va[c + step])); deg += 1.0; }
    }
    *rhs = r * inv_s2;
    *diag = deg + alpha_s * ((double)W[c] / NWO_W_ONE);
}

// S of a node: 0 plus the present neighbours in the order -x +x -y +y -z +z
NWO_HD double nwo_neighbour_sum(const double *chi, int level, int i, int j, int k)
{
    const int n = 1 << level;
    const int64_t c = nwo_lin(level, i, j, k), sy = (int64_t)1 << level, sz = (int64_t)1 << (2 * level);
    double S = 0.0;
    if (i > 0) S += chi[c - 1];
    if (i < n - 1) S += chi[c + 1];
    if (j > 0) S += chi[c - sy];
    if (j < n - 1) S += chi[c + sy];
    if (k > 0) S += chi[c - sz];
    if (k < n - 1) S += chi[c + sz];
    return S;
}

NWO_HD double nwo_update(double rhs, double S, double diag) { return (rhs + S) / diag; }

NWO_HD double nwo_residual(double rhs, double diag, double chi, double S) { return fabs(rhs - (diag * chi - S)); }

// ---- prolongation -------------------------------------------------------------------------------------------------------------------------
NWO_HD double nwo_mix(double near, double far) { return 0.75 * near + 0.25 * far; }

// node (i, j, k) of level `level` from the level below it: x, then y, then z
NWO_HD double nwo_prolong_node(const double *a, int level, int i, int j, int k)
{
    const int lc = level - 1, nc = 1 << lc;
    const int I0 = i >> 1, J0 = j >> 1, K0 = k >> 1;
    int I1 = I0 + ((i & 1) ? 1 : -1), J1 = J0 + ((j & 1) ? 1 : -1), K1 = K0 + ((k & 1) ? 1 : -1);
    I1 = I1 < 0 ? 0 : I1 > nc - 1 ? nc - 1 : I1;
    J1 = J1 < 0 ? 0 : J1 > nc - 1 ? nc - 1 : J1;
    K1 = K1 < 0 ? 0 : K1 > nc - 1 ? nc - 1 : K1;
    const double x00 = nwo_mix(a[nwo_lin(lc, I0, J0, K0)], a[nwo_lin(lc, I1, J0, K0)]);
    const double x10 = nwo_mix(a[nwo_lin(lc, I0, J1, K0)], a[nwo_lin(lc, I1, J1, K0)]);
    const double x01 = nwo_mix(a[nwo_lin(lc, I0, J0, K1)], a[nwo_lin(lc, I1, J0, K1)]);
    const double x11 = nwo_mix(a[nwo_lin(lc, I0, J1, K1)], a[nwo_lin(lc, I1, J1, K1)]);
    return nwo_mix(nwo_mix(x00, x10), nwo_mix(x01, x11));
}

// ---- the field ----------------------------------------------------------------------------------------------------------------------------
// the smallest power of two >= m, m > 0 and finite
NWO_HD double nwo_pow2_above(double m)
{
    int e = 0;
    const double f = frexp(m, &e);
    return f == 0.5 ? m : ldexp(1.0, e);
}

NWO_HD uint64_t nwo_quantise(double chi, double E) { return (uint64_t)(rint((chi / E) * NWO_F_HALF) + NWO_F_HALF); }

// floor(sum W F / sum W) from the limb sums, sum_w > 0 (128-bit arithmetic; the host calls it)
NWO_HD uint64_t nwo_level(uint64_t lo_sum, uint64_t hi_sum, uint64_t sum_w)
{
    const unsigned __int128 num = ((unsigned __int128)hi_sum << 16) + (unsigned __int128)lo_sum;
    return (uint64_t)(num / (unsigned __int128)sum_w);
}

#endif
