// kernels_train2.h -- second-order part of the fine-tuning backward (stage B): the parameter
// gradient of a loss that depends on FORCES and STRESS (reference: loss.backward() through the
// create_graph=True force / stress of chgnet/model/model.py:517-535, trainer.py:399-411).
//
// Derivation (checked in float64 against torch double-backward by the tests' pipeline model):
//   dL/d theta = d/d theta [ sum_b ce_b E_b + D E ],   D E = d/d tau E(v + tau vdot),
//   vdot_e = ux[c_e] - ux[n_e] + v_e W_b,  ux = -dL/dF,  W_b = (kappa / V_b) dL/d sigma_b.
// One tangent (forward-mode) sweep gives the tangent of every activation; the reverse sweep then carries TWO
// adjoints per activation: G(y) = dE/dy (seed 1) and bar(y) = d Phi / dy (seed ce), with
//   bar(x) = J^T bar(y) + d/dx [G(y) . J(x) xdot],    bar(W) += bar(y) x^T + G(y) xdot^T.
//
// Per layer the sweep runs as fused tile kernels (kernels_train2_tile.h, kernels_train2_freq.h).  What is here: the row-local
// nonlinear pieces those kernels share -- LayerNorm statistics and the gated-MLP tail with its tangent and two-adjoint backward, one
// row at a time, lane f = feature f of the core branch and of the gate branch ([rows][128] rows: columns 0..63 core, 64..127 gate) --
// and the row-parallel kernels of the geometry tangent, the bases, the embedding linears and the readout.
#pragma once

#include "kernels_geom.h"
#include "mfma_tile.h"

namespace chg {

__device__ __forceinline__ float wmean64(float v) { return wave_sum(v) * (1.0f / 64.0f); }

// silu''(x) and sigmoid''(x)
__device__ __forceinline__ float ddsiluf_(float x) {
  const float s = sigmoidf_(x);
  return s * (1.0f - s) * (2.0f + x * (1.0f - 2.0f * s));
}

struct LnRow { float xh, rstd; };
__device__ __forceinline__ LnRow ln_row(float x) {   // LayerNorm statistics of a 64-vector held one element per lane
  const float mu = wmean64(x);
  const float xc = x - mu;
  const float rstd = __builtin_amdgcn_rsqf(wmean64(xc * xc) + LN_EPS);
  return LnRow{xc * rstd, rstd};
}
// P(a) = a - mean(a) - xhat mean(a xhat);  m_ax returns mean(a xhat)
__device__ __forceinline__ float ln_proj(float a, float xh, float& m_ax) {
  const float ma = wmean64(a);
  m_ax = wmean64(a * xh);
  return a - ma - xh * m_ax;
}

// ---------------------------------------------------------------------------------------------------------
// gated MLP tail:  (c, g) -> y = silu(LN1 c) * sigmoid(LN2 g), forward with tangent and the two-adjoint backward
// ---------------------------------------------------------------------------------------------------------
// Per layer (pre-activations from the layer's tables, kernels_train2_tile.h; tangents alike, Pd / Qd / Rd / Sd):
//   AtomConv    z = P[centre][0:128] + P[nbr][128:256] + Q[bond],  h = silu(z), hd = silu'(z) zd,  c|g = h . [W2c | W2g]^T + b2
//   BondConv    z = R[b1][0:128] + R[b2][128:256] + S[ctr] + ang . W_ang^T, then as AtomConv
//   AngleUpdate c|g = z of BondConv's form (a single layer)
// and y = silu(LN1 c) * sigmoid(LN2 g) (gated_row_fwd) leaves the row as
//   AtomConv    m = y wag[k], summed into the aggregate of the centre:  md = yd wag + y wagd
//   BondConv    u = y wbg[b1] wbg[b2], summed into the aggregate of bond b1:  ud = yd w1 w2 + y (w1d w2 + w1 w2d)
//   AngleUpdate ang' = ang + y
// The two adjoints of y that gated_row_bwd takes, from those of the aggregate row a (bar(a), G(a)):
//   AtomConv    bar(y) = wag bar(a) + wagd G(a),  G(y) = wag G(a);   bar(wag) += y bar(a) + yd G(a)
//   BondConv    bar(y) = w1 w2 bar(a) + (w1d w2 + w1 w2d) G(a),  G(y) = w1 w2 G(a);
//               bar(w1) += y w2 bar(a) + (yd w2 + y w2d) G(a),  bar(w2) += y w1 bar(a) + (yd w1 + y w1d) G(a)
//   AngleUpdate bar(y) = bar(ang'),  G(y) = G(ang')
// (G(wag), G(wbg) are first-order adjoints: the force sweep leaves them in the batch.)
struct GatedRow {       // everything the backward needs of one row, this lane's feature
  float xh1, r1, xh2, r2, xh1d, xh2d, n1d, n2d, a1, a2, a1d, a2d, da1, da2, s1, n1;
  float pt1, pt2, mt1, mt2;   // P(cd), P(gd), mean(cd xh1), mean(gd xh2)
  float y, yd;
};

__device__ __forceinline__ GatedRow gated_row_fwd(float c, float g, float cd, float gd, float g1, float b1, float g2, float b2) {
  GatedRow s;
  const LnRow l1 = ln_row(c), l2 = ln_row(g);
  s.xh1 = l1.xh; s.r1 = l1.rstd; s.xh2 = l2.xh; s.r2 = l2.rstd;
  s.pt1 = ln_proj(cd, s.xh1, s.mt1);
  s.pt2 = ln_proj(gd, s.xh2, s.mt2);
  s.xh1d = s.r1 * s.pt1;
  s.xh2d = s.r2 * s.pt2;
  s.n1 = g1 * s.xh1 + b1;
  const float n2 = g2 * s.xh2 + b2;
  s.n1d = g1 * s.xh1d;
  s.n2d = g2 * s.xh2d;
  s.s1 = sigmoidf_(s.n1);
  s.a1 = s.n1 * s.s1;
  s.da1 = s.s1 * (1.0f + s.n1 * (1.0f - s.s1));
  s.a2 = sigmoidf_(n2);
  s.da2 = s.a2 * (1.0f - s.a2);
  s.a1d = s.da1 * s.n1d;
  s.a2d = s.da2 * s.n2d;
  s.y = s.a1 * s.a2;
  s.yd = s.a1d * s.a2 + s.a1 * s.a2d;
  return s;
}

// bar(y), G(y) -> bar(c), bar(g), G(c), G(g); lnacc[8] += LayerNorm-affine gradients of this lane's feature
__device__ __forceinline__ void gated_row_bwd(const GatedRow& s, float bar_y, float g_y, float g1, float g2, float (&lnacc)[4],
                                              float& bar_c, float& bar_g, float& g_c, float& g_g) {
  const float bar_a1 = s.a2 * bar_y + s.a2d * g_y, bar_a2 = s.a1 * bar_y + s.a1d * g_y;
  const float g_a1 = s.a2 * g_y, g_a2 = s.a1 * g_y;
  const float dda1 = s.s1 * (1.0f - s.s1) * (2.0f + s.n1 * (1.0f - 2.0f * s.s1));
  const float dda2 = s.da2 * (1.0f - 2.0f * s.a2);
  const float bar_n1 = s.da1 * bar_a1 + dda1 * s.n1d * g_a1, g_n1 = s.da1 * g_a1;
  const float bar_n2 = s.da2 * bar_a2 + dda2 * s.n2d * g_a2, g_n2 = s.da2 * g_a2;
  lnacc[0] += bar_n1 * s.xh1 + g_n1 * s.xh1d;
  lnacc[1] += bar_n1;
  lnacc[2] += bar_n2 * s.xh2 + g_n2 * s.xh2d;
  lnacc[3] += bar_n2;
  {   // LayerNorm 1
    const float h = g1 * g_n1;
    float m_hx, m_bx;
    const float ph = ln_proj(h, s.xh1, m_hx);
    const float pb = ln_proj(g1 * bar_n1, s.xh1, m_bx);
    const float m_hpt = wmean64(h * s.pt1);
    bar_c = s.r1 * pb - s.r1 * s.r1 * (s.xh1 * m_hpt + ph * s.mt1 + s.pt1 * m_hx);
    g_c = s.r1 * ph;
  }
  {   // LayerNorm 2
    const float h = g2 * g_n2;
    float m_hx, m_bx;
    const float ph = ln_proj(h, s.xh2, m_hx);
    const float pb = ln_proj(g2 * bar_n2, s.xh2, m_bx);
    const float m_hpt = wmean64(h * s.pt2);
    bar_g = s.r2 * pb - s.r2 * s.r2 * (s.xh2 * m_hpt + ph * s.mt2 + s.pt2 * m_hx);
    g_g = s.r2 * ph;
  }
}

// hidden layer:  bar(z) = silu'(z) bar(H) + silu''(z) zd G(H),   G(z) = silu'(z) G(H)      (elementwise over [rows,128])
static __global__ void k2_hidden_b(const float* __restrict__ Z, const float* __restrict__ Zd, const float* __restrict__ BH,
                            const float* __restrict__ GH, float* __restrict__ BZ, float* __restrict__ GZ, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float z = Z[i], d1 = dsiluf_(z), gh = GH[i];
  BZ[i] = d1 * BH[i] + ddsiluf_(z) * Zd[i] * gh;
  GZ[i] = d1 * gh;
}

// ---------------------------------------------------------------------------------------------------------
// geometry: tangent of the bond vectors
// ---------------------------------------------------------------------------------------------------------
// vd_e = ux[c] - ux[n] + v_e W_b;  rd = u . vd;  ud = (vd - u rd) / r          out: vd4 = (vd, rd), ud4 = (ud, 0)
static __global__ void k2_geom_t(const f32x4* __restrict__ ev, const f32x4* __restrict__ eu, const int* __restrict__ e_center,
                          const int* __restrict__ e_nbr, const int* __restrict__ e_owner, const float* __restrict__ ux,
                          const float* __restrict__ Wst, f32x4* __restrict__ vd4, f32x4* __restrict__ ud4, int n_edges) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const f32x4 v = ev[e], u = eu[e];
  const float* W = Wst + 9 * (size_t)e_owner[e];
  const int c = e_center[e], n = e_nbr[e];
  float vd[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) vd[k] = ux[3 * c + k] - ux[3 * n + k] + v[0] * W[k] + v[1] * W[3 + k] + v[2] * W[6 + k];
  const float rd = u[0] * vd[0] + u[1] * vd[1] + u[2] * vd[2];
  const float inv_r = 1.0f / v[3];
  vd4[e] = f32x4{vd[0], vd[1], vd[2], rd};
  ud4[e] = f32x4{(vd[0] - u[0] * rd) * inv_r, (vd[1] - u[1] * rd) * inv_r, (vd[2] - u[2] * rd) * inv_r, 0.f};
}

// ---------------------------------------------------------------------------------------------------------
// radial / Fourier bases with tangents, the 31 -> 64 embedding linears, and the frequency gradients
// ---------------------------------------------------------------------------------------------------------
// rbf value and its r-, f- and mixed derivatives (basis.py:108-116, 197-206)
__device__ __forceinline__ void rbf_all(float r, float rc, float freq, Envelope env, float& val, float& dr, float& df, float& drdf) {
  const float inv_rc = 1.0f / rc, w = freq * inv_rc, cn = sqrtf(2.0f * inv_rc);
  float sn, cs;
  sincos_cw(w * r, sn, cs);
  const float s = r * inv_rc;
  float e = 0.f, de = 0.f;
  if (s < 1.0f) {
    const float sp1 = ipow(s, env.p - 1), sp = sp1 * s;
    e = 1.0f + env.a * sp + env.b * sp * s + env.c * sp * s * s;
    de = (env.a * env.p * sp1 + env.b * (env.p + 1) * sp + env.c * (env.p + 2) * sp * s) * inv_rc;
  }
  val = e * cn * sn / r;
  dr = de * cn * sn / r + e * cn * (w * cs / r - sn / (r * r));
  df = e * cn * cs * inv_rc;
  drdf = cn * inv_rc * (de * cs - e * w * sn);
}

constexpr int KB2 = 32;   // basis count padded

struct BondBasisArgs {
  int n_und;
  const f32x4 *ev, *vd4;
  const int* u_u2d;
  const float *freq_ag, *freq_bg;
  float rc_ag, rc_bg;
  Envelope env;
  float *X6, *X6d, *X3, *X3d;     // [Eu,32]: basis and tangent (column 31 = 0)
};

static __global__ void k2_bond_basis(BondBasisArgs p) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = t / KB2, j = t % KB2;
  if (k >= p.n_und) return;
  const int e = p.u_u2d[k];
  const float r = p.ev[e][3], rd = p.vd4[e][3];
  float v6 = 0.f, d6 = 0.f, v3 = 0.f, d3 = 0.f, df, drdf;
  if (j < NRAD) {
    rbf_all(r, p.rc_ag, p.freq_ag[j], p.env, v6, d6, df, drdf);
    rbf_all(r, p.rc_bg, p.freq_bg[j], p.env, v3, d3, df, drdf);
  }
  p.X6[t] = v6; p.X6d[t] = d6 * rd; p.X3[t] = v3; p.X3d[t] = d3 * rd;
}

// out[row][f] = sum_j W[f][j] X[row][j]  (W [64][31] row-major, X [rows][32]); optional output row map
static __global__ __launch_bounds__(256) void k2_embed_lin(const float* __restrict__ X, const float* __restrict__ W, float* __restrict__ out,
                                                    const int* __restrict__ in_rows, int rows) {
  __shared__ float Ws[D * NRAD];
  for (int i = threadIdx.x; i < D * NRAD; i += blockDim.x) Ws[i] = W[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int r = wave; r < rows; r += nwaves) {
    const size_t src = (size_t)(in_rows ? in_rows[r] : r) * KB2;
    const float x = lane < KB2 ? X[src + lane] : 0.f;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NRAD; ++j) acc += Ws[lane * NRAD + j] * bcast(x, j);
    out[(size_t)r * D + lane] = acc;
  }
}

// Fourier basis of every angle with tangent:  X [A,32], Xd [A,32];  also theta and thetadot (for the frequency gradient)
static __global__ void k2_angle_basis(const f32x4* __restrict__ eu, const f32x4* __restrict__ ud4, const int* __restrict__ a_d1,
                               const int* __restrict__ a_d2, const float* __restrict__ freq, float* __restrict__ X, float* __restrict__ Xd,
                               float* __restrict__ th2, int n_angles) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int a = t / KB2, j = t % KB2;
  if (a >= n_angles) return;
  const f32x4 u1 = eu[a_d1[a]], u2 = eu[a_d2[a]], v1 = ud4[a_d1[a]], v2 = ud4[a_d2[a]];
  const float cosv = (u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2]) * KAPPA;
  const float cosd = (v1[0] * u2[0] + v1[1] * u2[1] + v1[2] * u2[2] + u1[0] * v2[0] + u1[1] * v2[1] + u1[2] * v2[2]) * KAPPA;
  const float theta = acosf(cosv), thd = -cosd / sqrtf(1.0f - cosv * cosv);
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

// ---------------------------------------------------------------------------------------------------------
// readout: LayerNorm and the three silu layers, tangent forward and two-adjoint backward (rows = atoms, width 64)
// ---------------------------------------------------------------------------------------------------------
// LayerNorm forward with tangent:  y = gamma xhat + beta,  yd = gamma xhatd;  keeps xhat, xhatd, rstd (per row in R[3*row..])
static __global__ __launch_bounds__(256) void k2_ln_t(const float* __restrict__ x, const float* __restrict__ xd, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, float* __restrict__ y, float* __restrict__ yd,
                                               float* __restrict__ xh, float* __restrict__ xhd, int rows) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  const float g = gamma[lane], b = beta[lane];
  for (int r = wave; r < rows; r += nwaves) {
    const size_t o = (size_t)r * D + lane;
    const LnRow l = ln_row(x[o]);
    float m;
    const float hd = l.rstd * ln_proj(xd[o], l.xh, m);
    y[o] = g * l.xh + b; yd[o] = g * hd; xh[o] = l.xh; xhd[o] = hd;
  }
}

// bar(y), G(y) -> bar(x), G(x) through the LayerNorm; dgam / dbet rows are written for a later column sum
static __global__ __launch_bounds__(256) void k2_ln_b(const float* __restrict__ x, const float* __restrict__ xd, const float* __restrict__ gamma,
                                               const float* __restrict__ bar_y, const float* __restrict__ g_y, float* __restrict__ bar_x,
                                               float* __restrict__ g_x, float* __restrict__ dgam, float* __restrict__ dbet, int rows) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  const float g = gamma[lane];
  for (int r = wave; r < rows; r += nwaves) {
    const size_t o = (size_t)r * D + lane;
    const LnRow l = ln_row(x[o]);
    float mt, m_hx, m_bx;
    const float pt = ln_proj(xd[o], l.xh, mt);
    const float by = bar_y[o], gy = g_y[o];
    const float h = g * gy;
    const float ph = ln_proj(h, l.xh, m_hx);
    const float pb = ln_proj(g * by, l.xh, m_bx);
    const float m_hpt = wmean64(h * pt);
    bar_x[o] = l.rstd * pb - l.rstd * l.rstd * (l.xh * m_hpt + ph * mt + pt * m_hx);
    g_x[o] = l.rstd * ph;
    dgam[o] = by * l.xh + gy * l.rstd * pt;
    dbet[o] = by;
  }
}

// s = silu(l), sd = silu'(l) ld
static __global__ void k2_silu_t(const float* __restrict__ l, const float* __restrict__ ld, float* __restrict__ s, float* __restrict__ sd, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  s[i] = siluf_(l[i]);
  sd[i] = dsiluf_(l[i]) * ld[i];
}

// seeds of the reverse sweep at the site energies:  bar(s3) = cot[owner] w3,  G(s3) = w3;  also d w3 rows = cot s3 + s3d
static __global__ void k2_readout_seed(const float* __restrict__ w3, const float* __restrict__ cot, const int* __restrict__ owner,
                                const float* __restrict__ s3, const float* __restrict__ s3d, float* __restrict__ bar_s,
                                float* __restrict__ g_s, float* __restrict__ dw3_rows, int n_atoms) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_atoms * D) return;
  const int i = t / D, f = t % D;
  const float c = cot[owner[i]];
  bar_s[t] = c * w3[f];
  g_s[t] = w3[f];
  dw3_rows[t] = c * s3[t] + s3d[t];
}

}  // namespace chg
