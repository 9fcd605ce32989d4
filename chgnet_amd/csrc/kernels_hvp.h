// kernels_hvp.h -- exact Hessian-vector products (chg_hessian_vector): the x-gradient of  Edot = grad E . u  at the embedding level.
//
// The HVP mode of the second-order sweep (engine_train.hip run_backward2) leaves, for every basis row, bar(basis) (adjoint of the
// primal) and G(basis) (adjoint of the tangent) through the 31 -> 64 embedding linears.  Edot depends on the positions only through
// the geometry (bond length r and its tangent rdot, angle theta and thetadot), so
//
//   per bond:   s = sum_j [ bar_j dX_j/dr + G_j d2X_j/dr2 rdot ]    (adjoint of r)        t = sum_j G_j dX_j/dr   (adjoint of rdot)
//   per angle:  the same in theta / thetadot, then chained through theta = acos(kappa u1.u2) to the two edges' unit vectors and their
//               tangents in float64: at collinear triplets 1 - kappa^2 c^2 ~ 2e-6, where the 1/sin(theta) terms of the second derivative
//               dominate and the float32 1 - c*c loses several percent.
//
// The results are emitted as k_edge_force's operands (kernels_geom.h): Grk[k] += adjoint of r_k (every radial component of a bond, from
// either of its directed edges: the reverse edge's radial part equals the representative's), Gu[e] += r_e x (transverse adjoint of v_e),
// so that kernel's  gv_e = Grk u_e + (I - u u^T) Gu_e / r_e  is the adjoint of the bond vector v_e = x_c - x_n and its "force" is -H u.
// The contractions with W^T run on the matrix pipe on 16-row tiles (embed_adjoint), the layout of kernels_train2_freq.h.
//
// Strain blocks (chg_hessian_vector_strain): E(x, eps) with every bond vector v_e = v0_e (I + eps) (lattice L (I + eps), fixed
// fractional coordinates), direction (u, W).  The tangent sweep already takes W (k2_geom_t: vd_e = u_c - u_n + v_e W), so the
// second-order adjoint gv2_e above is the same; what differs is the chain back to (x, eps) -- k_hvp_strain_scatter.
#pragma once

#include "kernels_embed.h"
#include "kernels_geom.h"
#include "kernels_train2.h"

namespace chg {

constexpr double HVP_KAPPA = 1.0 - 1e-6;    // encoders.py:144, in float64 here

// rbf first and second r-derivatives (basis.py:108-116, 197-206):  X = e(r) cn sin(w r) / r
__device__ __forceinline__ void rbf_d12(float r, float rc, float freq, Envelope env, float& d1, float& d2) {
  const float inv_rc = 1.0f / rc, w = freq * inv_rc, cn = sqrtf(2.0f * inv_rc);
  float sn, cs;
  sincos_cw(w * r, sn, cs);
  const float s = r * inv_rc;
  float e = 0.f, de = 0.f, dde = 0.f;
  if (s < 1.0f) {
    const int p = env.p;
    const float sp2 = p >= 2 ? ipow(s, p - 2) : 1.0f / s, sp1 = sp2 * s, sp = sp1 * s;
    e = 1.0f + env.a * sp + env.b * sp * s + env.c * sp * s * s;
    de = (env.a * p * sp1 + env.b * (p + 1) * sp + env.c * (p + 2) * sp * s) * inv_rc;
    dde = (env.a * p * (p - 1) * sp2 + env.b * (p + 1) * p * sp1 + env.c * (p + 2) * (p + 1) * sp) * inv_rc * inv_rc;
  }
  const float ir = 1.0f / r;
  const float g0 = sn * ir, g1 = (w * cs - sn * ir) * ir, g2 = (-w * w * sn - 2.0f * w * cs * ir + 2.0f * sn * ir * ir) * ir;
  d1 = cn * (de * g0 + e * g1);
  d2 = cn * (dde * g0 + 2.0f * de * g1 + e * g2);
}

// float64 geometry of one angle: unit vectors, their tangents, c = u1.u2, its tangent, and S = sqrt(1 - kappa^2 c^2) formed as
// (1 - kappa^2) + kappa^2 |u1 x u2|^2 (no cancellation at collinearity)
struct AngleGeom64 {
  double u1[3], u2[3], ud1[3], ud2[3], v1d[3], v2d[3], r1, r2, rd1, rd2, c, cd, S;
};

__device__ __forceinline__ void angle_geom64(const f32x4* __restrict__ ev, const f32x4* __restrict__ vd4, int d1, int d2, AngleGeom64& q) {
  const f32x4 a = ev[d1], b = ev[d2], ad = vd4[d1], bd = vd4[d2];
  double v1[3] = {a[0], a[1], a[2]}, v2[3] = {b[0], b[1], b[2]};
  q.r1 = sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]);
  q.r2 = sqrt(v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2]);
  q.rd1 = 0.0; q.rd2 = 0.0;
  for (int k = 0; k < 3; ++k) {
    q.u1[k] = v1[k] / q.r1; q.u2[k] = v2[k] / q.r2;
    q.v1d[k] = ad[k]; q.v2d[k] = bd[k];
  }
  for (int k = 0; k < 3; ++k) { q.rd1 += q.u1[k] * q.v1d[k]; q.rd2 += q.u2[k] * q.v2d[k]; }
  q.c = 0.0; q.cd = 0.0;
  for (int k = 0; k < 3; ++k) {
    q.ud1[k] = (q.v1d[k] - q.u1[k] * q.rd1) / q.r1;
    q.ud2[k] = (q.v2d[k] - q.u2[k] * q.rd2) / q.r2;
    q.c += q.u1[k] * q.u2[k];
  }
  for (int k = 0; k < 3; ++k) q.cd += q.ud1[k] * q.u2[k] + q.u1[k] * q.ud2[k];
  const double x0 = q.u1[1] * q.u2[2] - q.u1[2] * q.u2[1], x1 = q.u1[2] * q.u2[0] - q.u1[0] * q.u2[2], x2 = q.u1[0] * q.u2[1] - q.u1[1] * q.u2[0];
  const double k2 = HVP_KAPPA * HVP_KAPPA;
  q.S = sqrt((1.0 - k2) + k2 * (x0 * x0 + x1 * x1 + x2 * x2));
}

// Fourier basis of every angle with its tangent in the HVP mode: what k2_angle_basis forms, with theta and thetadot from the float64
// geometry (thetadot = -kappa cdot / S is exact at collinearity, where the float32 form divides by a 1 - c*c that lost several percent)
static __global__ void k_hvp_angle_basis(const f32x4* __restrict__ ev, const f32x4* __restrict__ vd4, const int* __restrict__ a_d1,
                                         const int* __restrict__ a_d2, const float* __restrict__ freq, float* __restrict__ X,
                                         float* __restrict__ Xd, float* __restrict__ th2, int n_angles) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int a = t / KB2, j = t % KB2;
  if (a >= n_angles) return;
  AngleGeom64 q;
  angle_geom64(ev, vd4, a_d1[a], a_d2[a], q);
  const float theta = (float)atan2(q.S, HVP_KAPPA * q.c), thd = (float)(-HVP_KAPPA * q.cd / q.S);
  float x = 0.f, dx = 0.f;
  if (j == 0) {
    x = INV_SQRT_2 * INV_SQRT_PI;
  } else if (j <= NFREQ) {
    float sn, cs;
    sincos_cw(freq[j - 1] * theta, sn, cs);
    x = sn * INV_SQRT_PI; dx = freq[j - 1] * cs * INV_SQRT_PI;
  } else if (j < NANG) {
    float sn, cs;
    sincos_cw(freq[j - 1 - NFREQ] * theta, sn, cs);
    x = cs * INV_SQRT_PI; dx = -freq[j - 1 - NFREQ] * sn * INV_SQRT_PI;
  }
  X[t] = x;
  Xd[t] = dx * thd;
  if (j == 0) { th2[2 * a] = theta; th2[2 * a + 1] = thd; }
}

struct HvpBondArgs {
  int rows;                       // bonds (atom-graph cutoff: all Eu; bond-graph cutoff: the Eb node bonds)
  const int* row_und;             // null: row k is undirected bond k; else undirected index of row
  const f32x4 *ev, *vd4;
  const int* u_u2d;
  const float* freq;              // [31]
  float rc;
  Envelope env;
  const float *barA, *gA, *WA;    // adjoint rows [rows,64] and their [64][31] weight
  const float *barB, *gB, *WB;    // optional second pair (null)
  float* Gu;                      // [Ed,4]  += t vdot of the representative edge
  float* Grk;                     // [Eu]    += s
};

constexpr size_t hvp_bond_lds() { return sizeof(float) * (2 * D * WSB + WAVES * TILE_ROWS * ETS); }

// sum over the four lanes (g = 0..3) that hold one row's 31 basis columns
__device__ __forceinline__ float sum_over_g(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

static __global__ __launch_bounds__(BLOCK) void k_hvp_bond_t(HvpBondArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Wa = smem;
  float* Wb = Wa + D * WSB;
  float* tiles = Wb + D * WSB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
  stage_embed_split_t(reinterpret_cast<h16x8*>(Wa), p.WA, tid);
  if (p.WB) stage_embed_split_t(reinterpret_cast<h16x8*>(Wb), p.WB, tid);
  float fq[2][4];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 16 * kt + 4 * g + r;
      fq[kt][r] = k < NRAD ? p.freq[k] : 0.f;
    }
  __syncthreads();
  float* T = tiles + wave * TILE_ROWS * ETS;
  float* Trow = T + j * ETS;
  const int ntiles = (p.rows + BLOCK_ROWS - 1) / BLOCK_ROWS;
  int tb, te;
  tile_range(ntiles, tb, te);
  for (int tile = tb; tile < te; ++tile) {
    const int row0 = tile * BLOCK_ROWS + wave * TILE_ROWS;
    const int nvalid = min(TILE_ROWS, p.rows - row0);
    if (nvalid <= 0) continue;
    const bool valid = j < nvalid;
    const int row = row0 + (valid ? j : 0);
    const int und = p.row_und ? p.row_und[row] : row;
    const int e = p.u_u2d[und];
    const f32x4 vd = p.vd4[e];
    const float rr = p.ev[e][3], rd = vd[3];
    f32x4 tb_[2] = {zero4(), zero4()}, tg_[2] = {zero4(), zero4()};
    V64 gin;
    auto contract = [&](const float* rows, const float* img, f32x4 (&t)[2]) {
      gather_rows64(T, ETS, rows, row, lane);
      __builtin_amdgcn_wave_barrier();
      read_dl<VT>(Trow, g, gin.t);
      embed_adjoint(t, img, gin, j, g);
      __builtin_amdgcn_wave_barrier();
    };
    contract(p.barA, Wa, tb_);
    contract(p.gA, Wa, tg_);
    if (p.WB) {
      contract(p.barB, Wb, tb_);
      contract(p.gB, Wb, tg_);
    }
    float s = 0.f, t = 0.f;
    if (valid) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (16 * kt + 4 * g + r >= NRAD) continue;
          float d1, d2;
          rbf_d12(rr, p.rc, fq[kt][r], p.env, d1, d2);
          s += tb_[kt][r] * d1 + tg_[kt][r] * d2 * rd;
          t += tg_[kt][r] * d1;
        }
    }
    s = sum_over_g(s);
    t = sum_over_g(t);
    if (valid && g == 0) {
      atomicAdd(p.Grk + und, s);
#pragma unroll
      for (int k = 0; k < 3; ++k) atomicAdd(p.Gu + 4 * (size_t)e + k, t * vd[k]);   // rdot = u . vdot: (I - u u^T) vdot / r is k_edge_force's
    }
  }
}

constexpr size_t hvp_angle_lds() { return sizeof(float) * (D * WSB + WAVES * TILE_ROWS * ETS); }

// per angle: adjoints of theta (sth) and thetadot (tth) from bar(ang0) / G(ang0) through the Fourier basis, then in float64 through
//   theta = acos(kappa c), thetadot = -kappa cdot / S,  c = u1.u2,  cdot = ud1.u2 + u1.ud2,  ud = (I - u u^T) vdot / r
// to the adjoint of each bond vector v (radial part -> Grk of its bond, transverse part x r -> Gu of the edge)
static __global__ __launch_bounds__(BLOCK) void k_hvp_angle_t(const float* __restrict__ bar_ang, const float* __restrict__ g_ang,
                                                              const float* __restrict__ Wae, const float* __restrict__ th2,
                                                              const float* __restrict__ freq, const f32x4* __restrict__ ev,
                                                              const f32x4* __restrict__ vd4, const int* __restrict__ a_d1,
                                                              const int* __restrict__ a_d2, const int* __restrict__ e_d2u,
                                                              float* __restrict__ Gu, float* __restrict__ Grk, int n_angles) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* We = smem;
  float* tiles = We + D * WSB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
  stage_embed_split_t(reinterpret_cast<h16x8*>(We), Wae, tid);
  float fq[2][4];
  int kind[2][4];      // 0 nothing, 1 sine column, 2 cosine column
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 16 * kt + 4 * g + r;
      kind[kt][r] = (k >= 1 && k <= NFREQ) ? 1 : ((k > NFREQ && k < NANG) ? 2 : 0);
      fq[kt][r] = kind[kt][r] == 1 ? freq[k - 1] : (kind[kt][r] == 2 ? freq[k - 1 - NFREQ] : 0.f);
    }
  __syncthreads();
  float* T = tiles + wave * TILE_ROWS * ETS;
  float* Trow = T + j * ETS;
  const int ntiles = (n_angles + BLOCK_ROWS - 1) / BLOCK_ROWS;
  int tb, te;
  tile_range(ntiles, tb, te);
  for (int tile = tb; tile < te; ++tile) {
    const int row0 = tile * BLOCK_ROWS + wave * TILE_ROWS;
    const int nvalid = min(TILE_ROWS, n_angles - row0);
    if (nvalid <= 0) continue;
    const bool valid = j < nvalid;
    const int a = row0 + (valid ? j : 0);
    const float theta = th2[2 * (size_t)a], thd = th2[2 * (size_t)a + 1];
    f32x4 tb_[2] = {zero4(), zero4()}, tg_[2] = {zero4(), zero4()};
    V64 gin;
    gather_rows64(T, ETS, bar_ang, a, lane);
    __builtin_amdgcn_wave_barrier();
    read_dl<VT>(Trow, g, gin.t);
    embed_adjoint(tb_, We, gin, j, g);
    __builtin_amdgcn_wave_barrier();
    gather_rows64(T, ETS, g_ang, a, lane);
    __builtin_amdgcn_wave_barrier();
    read_dl<VT>(Trow, g, gin.t);
    embed_adjoint(tg_, We, gin, j, g);
    __builtin_amdgcn_wave_barrier();
    float sth = 0.f, tth = 0.f;
    if (valid) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (kind[kt][r] == 0) continue;
          float sn, cs;
          sincos_cw(fq[kt][r] * theta, sn, cs);
          const float gq = fq[kt][r];
          // sine column: X' = g cos, X'' = -g^2 sin;  cosine column: X' = -g sin, X'' = -g^2 cos  (times 1/sqrt(pi))
          const float d1 = (kind[kt][r] == 1 ? gq * cs : -gq * sn) * INV_SQRT_PI;
          const float d2 = -gq * gq * (kind[kt][r] == 1 ? sn : cs) * INV_SQRT_PI;
          sth += tb_[kt][r] * d1 + tg_[kt][r] * d2 * thd;
          tth += tg_[kt][r] * d1;
        }
    }
    sth = sum_over_g(sth);
    tth = sum_over_g(tth);
    if (valid && g == 0) {
      const int d1 = a_d1[a], d2 = a_d2[a];
      AngleGeom64 q;
      angle_geom64(ev, vd4, d1, d2, q);
      const double K = HVP_KAPPA, iS = 1.0 / q.S;
      const double Acd = -K * (double)tth * iS;                                              // adjoint of cdot
      const double Ac = -K * (double)sth * iS - K * K * K * q.c * q.cd * (double)tth * iS * iS * iS;   // adjoint of c
      // c = u1.u2, cdot = ud1.u2 + u1.ud2:  adjoints of u1 (a1), ud1 (b1) and likewise for edge 2
      double a1[3], b1[3], a2[3], b2[3];
      for (int k = 0; k < 3; ++k) {
        a1[k] = Ac * q.u2[k] + Acd * q.ud2[k]; b1[k] = Acd * q.u2[k];
        a2[k] = Ac * q.u1[k] + Acd * q.ud1[k]; b2[k] = Acd * q.u1[k];
      }
      // u = v / r, ud = vdot / r - v (v . vdot) / r^3:  adjoint of v from (a, b)
      auto bond_adjoint = [&](const double* u, const double* vdd, double r, double rd, const double* aa, const double* bb, int e) {
        double au = 0.0, bu = 0.0, bv = 0.0;
        for (int k = 0; k < 3; ++k) { au += aa[k] * u[k]; bu += bb[k] * u[k]; bv += bb[k] * vdd[k]; }
        double gv[3], gr = 0.0;
        for (int k = 0; k < 3; ++k) {
          gv[k] = (aa[k] - au * u[k]) / r + (-bv * u[k] - bb[k] * rd - vdd[k] * bu + 3.0 * bu * rd * u[k]) / (r * r);
          gr += gv[k] * u[k];
        }
        atomicAdd(Grk + e_d2u[e], (float)gr);
        for (int k = 0; k < 3; ++k) atomicAdd(Gu + 4 * (size_t)e + k, (float)((gv[k] - gr * u[k]) * r));
      };
      bond_adjoint(q.u1, q.v1d, q.r1, q.rd1, a1, b1, d1);
      bond_adjoint(q.u2, q.v2d, q.r2, q.rd2, a2, b2, d2);
    }
  }
}

// ---- strain blocks: (x, eps)-adjoints of Edot = sum_e g_e . (u_c - u_n + v_e W) -> -hx [N,3] and hs [B,9] -------------------------------
// With g_e = dE/dv_e (the force sweep's operands, b->Gu / b->Grk) and gv2_e the second-order adjoint above (t.hvp_gu / t.hvp_grk):
//   x-adjoint of bond vector e:   gx_e = gv2_e + W g_e                   (the tangent's v0_e W term, chained through v0_e)
//   strain adjoint of owner b:    sum_e v_e (x) gv2_e + (u_c - u_n) (x) g_e
// d v_e / d eps . W = v0_e W does not depend on eps, so the virial has no v_e (x) W g_e term: the force and the virial see different
// per-edge operands, which k_edge_force cannot express.  Otherwise this is k_edge_force: the same centre-major segmented scatter of
// gx_rev(e) - gx_e (DPP scan, one atomic per run end) and the same per-wave / per-workgroup virial reduction, in fewer chunks per wave
// (twice the operands per edge).
struct HvpScatterArgs {
  const f32x4 *ev, *eu;
  const float *Gu2, *Grk2;    // second-order operands [Ed,4] [Eu]
  const float *Gu1, *Grk1;    // first-order operands of the force sweep [Ed,4] [Eu]
  const float *ux, *Wst;      // direction [N,3], [B,9]
  const int *e_center, *e_nbr, *e_d2u, *e_owner, *e_rev, *u_u2d;
  int n_edges;
  float* force;               // [N,3] zeroed: -hx
  float* virial;              // [B,9] zeroed: hs
};

constexpr int HVS_IT = 2;
constexpr int HVS_EDGES_PER_BLOCK = 4 * 64 * HVS_IT;

// dE/dv of edge e from k_edge_force's operands: gr u + (I - u u^T) gu / r  (gr: the bond's radial adjoint if e carries it, sign of u)
__device__ __forceinline__ void edge_grad(const f32x4& uu, float inv_r, float gr, const f32x4& gu, float (&gv)[3]) {
  const float dot = gu[0] * uu[0] + gu[1] * uu[1] + gu[2] * uu[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) gv[k] = gr * uu[k] + (gu[k] - dot * uu[k]) * inv_r;
}

static __global__ __launch_bounds__(256) void k_hvp_strain_scatter(HvpScatterArgs p) {
  __shared__ float vir[4][9];
  __shared__ int vown[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int base = (blockIdx.x * 4 + wave) * (64 * HVS_IT);
  int owner[HVS_IT];
#pragma unroll
  for (int it = 0; it < HVS_IT; ++it) {
    const int e = base + 64 * it + lane;
    owner[it] = e < p.n_edges ? p.e_owner[e] : -1;
  }
  float tv[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int first = __builtin_amdgcn_readfirstlane(owner[0]);
  bool uniform = first >= 0;
#pragma unroll
  for (int it = 0; it < HVS_IT; ++it) uniform = uniform && __all(owner[it] == first || owner[it] < 0) != 0;
#pragma unroll
  for (int it = 0; it < HVS_IT; ++it) {
    const int e = base + 64 * it + lane;
    const bool valid = e < p.n_edges;
    const int ec = valid ? e : 0;
    float d[3] = {0.f, 0.f, 0.f}, t9[9];
    int kcur = -1;
    {
      const f32x4 vr = p.ev[ec], uu = p.eu[ec];
      const int kk = p.e_d2u[ec], er = p.e_rev[ec], c = p.e_center[ec], n = p.e_nbr[ec];
      const bool rep = p.u_u2d[kk] == e;                    // lengths enter only via the representative edge of the bond
      const float g2r = p.Grk2[kk], g1r = p.Grk1[kk], inv_r = 1.0f / vr[3];
      const f32x4 mu = f32x4{-uu[0], -uu[1], -uu[2], 0.f}; // u_rev = -u
      float gv2[3], gv2r[3], g1[3], g1rv[3];
      edge_grad(uu, inv_r, rep ? g2r : 0.f, *reinterpret_cast<const f32x4*>(p.Gu2 + 4 * (size_t)ec), gv2);
      edge_grad(mu, inv_r, rep ? 0.f : g2r, *reinterpret_cast<const f32x4*>(p.Gu2 + 4 * (size_t)er), gv2r);
      edge_grad(uu, inv_r, rep ? g1r : 0.f, *reinterpret_cast<const f32x4*>(p.Gu1 + 4 * (size_t)ec), g1);
      edge_grad(mu, inv_r, rep ? 0.f : g1r, *reinterpret_cast<const f32x4*>(p.Gu1 + 4 * (size_t)er), g1rv);
      const float* W = p.Wst + 9 * (size_t)(valid ? owner[it] : 0);
      float du[3], dg[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) { du[k] = p.ux[3 * c + k] - p.ux[3 * n + k]; dg[k] = g1rv[k] - g1[k]; }
#pragma unroll
      for (int a = 0; a < 3; ++a) d[a] = gv2r[a] - gv2[a] + W[3 * a] * dg[0] + W[3 * a + 1] * dg[1] + W[3 * a + 2] * dg[2];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) t9[3 * a + b] = valid ? vr[a] * gv2[b] + du[a] * g1[b] : 0.f;
      if (!valid) d[0] = d[1] = d[2] = 0.f;
      kcur = valid ? c : -1;
    }
    // segmented inclusive scan over runs of equal centre (k_edge_force's)
    const int kprev = __builtin_amdgcn_update_dpp(-2, kcur, 0x138, 0xF, 0xF, false);    // wave_shr:1
    const unsigned long long heads = __ballot(lane == 0 || kprev != kcur);
    const int start = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));
#define CHG_SEG_STEP(ctrl, rmask, cond)                                                                                  \
    {                                                                                                                      \
      const float t0 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(d[0]), (ctrl), (rmask), 0xF, true)); \
      const float t1 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(d[1]), (ctrl), (rmask), 0xF, true)); \
      const float t2 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(d[2]), (ctrl), (rmask), 0xF, true)); \
      if (cond) {                                                                                                          \
        d[0] += t0;                                                                                                        \
        d[1] += t1;                                                                                                        \
        d[2] += t2;                                                                                                        \
      }                                                                                                                    \
    }
    const int row_lane = lane & 15, row_base = lane & ~15;
    CHG_SEG_STEP(0x111, 0xF, row_lane >= 1 && lane - 1 >= start)     // row_shr:1
    CHG_SEG_STEP(0x112, 0xF, row_lane >= 2 && lane - 2 >= start)     // row_shr:2
    CHG_SEG_STEP(0x114, 0xF, row_lane >= 4 && lane - 4 >= start)     // row_shr:4
    CHG_SEG_STEP(0x118, 0xF, row_lane >= 8 && lane - 8 >= start)     // row_shr:8
    CHG_SEG_STEP(0x142, 0xA, (row_base & 16) && start < row_base)    // row_bcast:15
    CHG_SEG_STEP(0x143, 0xC, row_base >= 32 && start < 32)           // row_bcast:31
#undef CHG_SEG_STEP
    const int knext = __builtin_amdgcn_update_dpp(-2, kcur, 0x130, 0xF, 0xF, false);    // wave_shl:1
    if (valid && (lane == 63 || knext != kcur)) {
#pragma unroll
      for (int k3 = 0; k3 < 3; ++k3) atomicAdd(p.force + 3 * (size_t)kcur + k3, d[k3]);
    }
    if (uniform) {
#pragma unroll
      for (int c = 0; c < 9; ++c) tv[c] += t9[c];
    } else {
      unsigned long long rem = __ballot(valid);
      while (rem) {
        const int o = __builtin_amdgcn_readlane(owner[it], __builtin_ctzll(rem));
        const bool mine = valid && owner[it] == o;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
          const float sck = wave_sum(mine ? t9[c] : 0.f);
          if (lane == 0) atomicAdd(p.virial + 9 * (size_t)o + c, sck);
        }
        rem &= ~__ballot(mine);
      }
    }
  }
  if (lane == 0) vown[wave] = uniform ? first : -2;
  if (uniform) {
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const float s = wave_sum(tv[c]);
      if (lane == 0) vir[wave][c] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const int c = threadIdx.x;
    int cur = -2;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int o = vown[w];
      if (o != cur) {
        if (cur >= 0) atomicAdd(p.virial + 9 * (size_t)cur + c, s);
        s = 0.f;
        cur = o;
      }
      if (o >= 0) s += vir[w][c];
    }
    if (cur >= 0) atomicAdd(p.virial + 9 * (size_t)cur + c, s);
  }
}

}  // namespace chg
