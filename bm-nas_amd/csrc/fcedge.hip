// Mixed-edge sums whose primitives include FC_Relu / FC_Mish (reference models/search/darts/operations.py:22-38,
// 48-65 inside FusionMixedOp.forward :104-105, summed over the incoming edges at model_search.py:58 and
// node_search.py:54):   out = sum_j sum_p w[j, p] OPS[p](x_j),
//   FC primitive:  u = W x + bias over channels,  a = relu(u) | u tanh(softplus(u)),  y = BatchNorm1d(a),  o = dropout(y).
// Every launch covers ALL edges of the sum (the edge is a grid dimension), so the launch count does not depend on n:
//   forward   fc_gemm_fwd_k   U_j = W_j^stack x_j + bias_j (fp32 MFMA 16x16x4), batch sums of a in the epilogue
//             fc_mix_fwd_k    BatchNorm finalisation in the launch + the streaming weighted sum (act recomputed from U)
//   backward  fc_bwd_reduce_k dw rows, dBN.weight / dBN.bias (the two sums the BatchNorm input gradient needs)
//             fc_bwd_du_k     dU = BatchNorm input gradient * act'(U), dbias
//             fc_bwd_gemm_k   dx = W^T dU + wskip g (edges reading one tensor share the destination: their K ranges are
//                             concatenated) and dW = dU x^T (split over the batch columns, atomics) as two block classes
// The per-edge pointers travel by value in the kernel arguments (uniform index -> scalar loads).
//
// FC edges of a FOUND network (reference models/search/darts/model.py:140-148 with operations.py:22-65): every edge keeps
// its own output, h_e = Dropout(BatchNorm1d(act_e(Linear_e(x_e)))) — no weight row, no skip term, no sum over edges,
// and the kind (ReLU | Mish) is per edge.  The two GEMM kernels above serve as they are (F = 1); the elementwise
// kernels come in "separate outputs" form with the edge as blockIdx.z:
//   forward   fc_sep_fwd_k         BatchNorm finalisation in the launch, out_e = drop_e(scale act_e(U_e) + shift)
//   backward  fc_sep_bwd_reduce_k  dBN.weight / dBN.bias of every edge from its own incoming gradient
//             fc_sep_bwd_du_k      dU_e = BatchNorm input gradient * act_e'(U_e), dbias_e
#include "drop_cfg.hpp"
#include "mish.hpp"

namespace {

constexpr int FC_E = BMNAS_FC_MAX_EDGES;
constexpr float FC_EPS = 1e-5f;
constexpr float FC_MOMENTUM = 0.1f;

// the activations act_f / dact_f / act4 / dact4 (ReLU | Mish): mish.hpp

__device__ __forceinline__ float skip_weight(const float* __restrict__ w, int j, int P, uint32_t skip_cols) {
  float s = 0.f;
  for (int p = 0; p < P; ++p)
    if ((skip_cols >> p) & 1u) s += w[j * P + p];
  return s;
}

// ------------------------------------------------------------------------------------------ forward GEMM
struct GemmFwdArgs {
  const float* x[FC_E];
  float* U[FC_E];
  const float* W[FC_E][2];
  const float* bias[FC_E][2];
  float* stat[FC_E][2];
  int mish[2];
};

// grid (column tiles of 64, row tiles of 64, edge); wave w of the block: rows 16 w .. 16 w + 15 of the row tile, 64
// columns.  A column is (sample, l); 16 columns hold whole samples (L <= 16), so one bound per column.
// K in chunks of 16: the lane's A operand is one float4 of its weight row (k = k0 + 4 slot + t for MFMA t — any
// bijection of k serves a sum), the B operand the matching 4 rows of the state.
__global__ __launch_bounds__(256) void fc_gemm_fwd_k(const GemmFwdArgs a, int F, int training, int b, int C, int lgL) {
  const int j = blockIdx.z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lo = lane & 15, h = lane >> 4;
  const int m0 = blockIdx.y * 64 + wave * 16;
  if (m0 >= F * C) return;
  const int L = 1 << lgL, N = b * L;
  const int f = m0 / C, mm = m0 - f * C;
  const float* __restrict__ W = a.W[j][f];
  const float* __restrict__ x = a.x[j];
  const int64_t CL = (int64_t)C * L;
  const int colbase = blockIdx.x * 64;
  const float* xp[4];
  bool cv[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int col = colbase + ct * 16 + lo;
    cv[ct] = col < N;
    const int cc = cv[ct] ? col : 0;
    xp[ct] = x + (int64_t)(cc >> lgL) * CL + (cc & (L - 1)) + (int64_t)(4 * h) * L;
  }
  f32x4 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* wp = W + (int64_t)(mm + lo) * C + 4 * h;
  for (int k0 = 0; k0 < C; k0 += 16) {
    const float4 a4 = ld4(wp + k0);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const float* p = xp[ct] + (int64_t)k0 * L;
      float b0 = p[0], b1 = p[L], b2 = p[2 * L], b3 = p[3 * L];
      if (!cv[ct]) b0 = b1 = b2 = b3 = 0.f;
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b0, acc[ct], 0, 0, 0);
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b1, acc[ct], 0, 0, 0);
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b2, acc[ct], 0, 0, 0);
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b3, acc[ct], 0, 0, 0);
    }
  }
  // acc[ct][r] = D[row m0 + 4 h + r][column colbase + 16 ct + lo]
  const float* __restrict__ bias = a.bias[j][f];
  float* __restrict__ U = a.U[j];
  const int mish = a.mish[f];
  const int64_t FCL = (int64_t)F * CL;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = mm + 4 * h + r;
    const float bv = bias[row];
    const float sh = act_f(bv, mish);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int col = colbase + ct * 16 + lo;
      if (cv[ct]) {
        const float u = acc[ct][r] + bv;
        U[(int64_t)(col >> lgL) * FCL + (int64_t)(f * C + row) * L + (col & (L - 1))] = u;
        const float d = act_f(u, mish) - sh;
        s1[r] += d;
        s2[r] += d * d;
      }
    }
  }
  if (training) {
    float* __restrict__ st = a.stat[j][f];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float t1 = row16_sum(s1[r]), t2 = row16_sum(s2[r]);
      if (lo == 0) {
        atomicAdd(st + mm + 4 * h + r, t1);
        atomicAdd(st + C + mm + 4 * h + r, t2);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ elementwise kernels
// A block of 256 threads works on 16 channels: a sample's 16-channel slab is 4 L float4s, 256 / (4 L) samples side by side.
struct Slab {
  int c, l0, sub, nsub, ch;      // channel, first l of the float4, sample slot, slots, channel within the tile
};
__device__ __forceinline__ Slab slab_of(int lgL) {
  const int lgq = lgL - 2;                 // float4s per row: L / 4
  const int lgs = lgq + 4;                 // float4s per slab
  const int t = threadIdx.x, r = t & ((1 << lgs) - 1);
  Slab s;
  s.sub = t >> lgs;
  s.nsub = 256 >> lgs;
  s.ch = r >> lgq;
  s.c = blockIdx.x * 16 + s.ch;
  s.l0 = (r & ((1 << lgq) - 1)) * 4;
  return s;
}
// sum of v over the threads of the block that share the calling thread's channel; valid in the threads with
// sub == 0 and l0 == 0 (one per channel).  red: 256 floats.
__device__ __forceinline__ float channel_sum(float v, const Slab& s, int lgL, float* red) {
  const int lgq = lgL - 2, lgs = lgq + 4;
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  float t = 0.f;
  if (s.sub == 0 && s.l0 == 0) {
    for (int u = 0; u < s.nsub; ++u)
      for (int q = 0; q < (1 << lgq); ++q) t += red[(u << lgs) + (s.ch << lgq) + q];
  }
  return t;
}

struct MixPrim {
  const float* stat;
  const float* bias;
  const float* bn_w;
  const float* bn_b;
  float* rm;
  float* rv;
  long long* nbt;
  float* chan;
};
struct MixArgs {
  const float* x[FC_E];
  const float* U[FC_E];
  MixPrim p[FC_E][2];
  uint64_t doff[FC_E][2];
  DropCfg drop;
  int mish[2];
  int col[2];
};

// grid (C / 16, ceil(b / nsub))
__global__ __launch_bounds__(256) void fc_mix_fwd_k(const MixArgs a, int n, int F, const float* __restrict__ w, int P,
                                                    uint32_t skip_cols, int training, float* __restrict__ out, int b,
                                                    int C, int lgL) {
  const Slab sl = slab_of(lgL);
  const int L = 1 << lgL;
  DropRt dr = drop_begin(a.drop);
  const uint64_t dbase = dr.off - a.drop.offset;       // the step counter alone; sites add their own offsets
  const int s = blockIdx.y * sl.nsub + sl.sub;
  const bool valid = s < b;
  const int sc = valid ? s : 0;
  const int c = sl.c;
  const int64_t e = ((int64_t)sc * C + c) * L + sl.l0;
  const bool writer = blockIdx.y == 0 && sl.sub == 0 && sl.l0 == 0;
  const float nN = (float)b * (float)L;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = 0; j < n; ++j) {
    if (skip_cols) {
      const float ws = skip_weight(w, j, P, skip_cols);
      const float4 x4 = ld4(a.x[j] + e);
      acc = f4_add(acc, f4_scale(x4, ws));
    }
    for (int f = 0; f < F; ++f) {
      const MixPrim& p = a.p[j][f];
      const int mish = a.mish[f];
      float mean, var, rstd;
      if (training) {
        const float md = p.stat[c] / nN;
        mean = act_f(p.bias[c], mish) + md;
        var = fmaxf(p.stat[C + c] / nN - md * md, 0.f);
      } else {
        mean = p.rm[c];
        var = p.rv[c];
      }
      rstd = rsqrtf(var + FC_EPS);
      const float scale = p.bn_w[c] * rstd, shift = p.bn_b[c] - mean * scale;
      if (writer) {
        p.chan[c] = mean;
        p.chan[C + c] = rstd;
        p.chan[2 * C + c] = scale;
        p.chan[3 * C + c] = shift;
        if (training) {
          p.rm[c] = (1.f - FC_MOMENTUM) * p.rm[c] + FC_MOMENTUM * mean;
          p.rv[c] = (1.f - FC_MOMENTUM) * p.rv[c] + FC_MOMENTUM * var * (nN / (nN - 1.f));
          if (blockIdx.x == 0 && threadIdx.x == 0 && p.nbt != nullptr) p.nbt[0] += 1;
        }
      }
      const float wf = w[j * P + a.col[f]];
      const float4 u4 = ld4(a.U[j] + ((int64_t)sc * F * C + f * C + c) * L + sl.l0);
      const float4 a4 = act4(u4, mish);
      dr.off = dbase + a.doff[j][f];
      const float4 dm = drop_mult4(dr, (uint64_t)e);
      acc.x += wf * dm.x * (scale * a4.x + shift);
      acc.y += wf * dm.y * (scale * a4.y + shift);
      acc.z += wf * dm.z * (scale * a4.z + shift);
      acc.w += wf * dm.w * (scale * a4.w + shift);
    }
  }
  if (valid) st4(out + e, acc);
}

struct BwdArgs {
  const float* x[FC_E];
  const float* U[FC_E];
  float* dU[FC_E];
  const float* chan[FC_E][2];
  float* bn_grad[FC_E][2];
  float* dbias[FC_E][2];
  uint64_t doff[FC_E][2];
  DropCfg drop;
  int mish[2];
  int col[2];
};

constexpr int FC_SPC = 32;       // samples per block of the backward's elementwise kernels (a multiple of every nsub)

// grid (C / 16, ceil(b / FC_SPC), edge)
__global__ __launch_bounds__(256) void fc_bwd_reduce_k(const BwdArgs a, int F, const float* __restrict__ w, int P,
                                                       uint32_t skip_cols, const float* __restrict__ g,
                                                       float* __restrict__ dw, int b, int C, int lgL) {
  __shared__ float red[256];
  const Slab sl = slab_of(lgL);
  const int L = 1 << lgL, j = blockIdx.z, c = sl.c;
  DropRt dr = drop_begin(a.drop);
  const uint64_t dbase = dr.off - a.drop.offset;
  const int s_end = min(b, (int)(blockIdx.y + 1) * FC_SPC);
  float mean[2], rstd[2], scale[2], shift[2], wf[2];
  for (int f = 0; f < F; ++f) {
    const float* ch = a.chan[j][f];
    mean[f] = ch[c]; rstd[f] = ch[C + c]; scale[f] = ch[2 * C + c]; shift[f] = ch[3 * C + c];
    wf[f] = w[j * P + a.col[f]];
  }
  float dwf[2] = {0.f, 0.f}, sdy[2] = {0.f, 0.f}, sda[2] = {0.f, 0.f}, dws = 0.f;
  for (int s = blockIdx.y * FC_SPC + sl.sub; s < s_end; s += sl.nsub) {
    const int64_t e = ((int64_t)s * C + c) * L + sl.l0;
    const float4 g4 = ld4(g + e);
    if (skip_cols) dws += f4_dot(g4, ld4(a.x[j] + e));
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      if (f < F) {
        const int mish = a.mish[f];
        const float4 a4 = act4(ld4(a.U[j] + ((int64_t)s * F * C + f * C + c) * L + sl.l0), mish);
        dr.off = dbase + a.doff[j][f];
        const float4 gm = f4_mul(g4, drop_mult4(dr, (uint64_t)e));       // mask * g
        const float4 y4 = make_float4(scale[f] * a4.x + shift[f], scale[f] * a4.y + shift[f],
                                      scale[f] * a4.z + shift[f], scale[f] * a4.w + shift[f]);
        dwf[f] += f4_dot(gm, y4);
        const float4 ah = make_float4((a4.x - mean[f]) * rstd[f], (a4.y - mean[f]) * rstd[f],
                                      (a4.z - mean[f]) * rstd[f], (a4.w - mean[f]) * rstd[f]);
        sdy[f] += wf[f] * f4_hsum(gm);
        sda[f] += wf[f] * f4_dot(gm, ah);
      }
    }
  }
  const bool lead = sl.sub == 0 && sl.l0 == 0;
  for (int f = 0; f < F; ++f) {
    const float t1 = channel_sum(sda[f], sl, lgL, red);
    const float t2 = channel_sum(sdy[f], sl, lgL, red);
    if (lead) {
      atomicAdd(a.bn_grad[j][f] + c, t1);
      atomicAdd(a.bn_grad[j][f] + C + c, t2);
    }
    const float t = block_sum256(dwf[f], red);
    if (threadIdx.x == 0) atomicAdd(dw + j * P + a.col[f], t);
  }
  if (skip_cols) {
    const float t = block_sum256(dws, red);
    if (threadIdx.x == 0)
      for (int p = 0; p < P; ++p)
        if ((skip_cols >> p) & 1u) atomicAdd(dw + j * P + p, t);
  }
}

// grid as fc_bwd_reduce_k
__global__ __launch_bounds__(256) void fc_bwd_du_k(const BwdArgs a, int F, const float* __restrict__ w, int P,
                                                   const float* __restrict__ g, int training, int b, int C, int lgL) {
  __shared__ float red[256];
  const Slab sl = slab_of(lgL);
  const int L = 1 << lgL, j = blockIdx.z, c = sl.c;
  DropRt dr = drop_begin(a.drop);
  const uint64_t dbase = dr.off - a.drop.offset;
  const int s_end = min(b, (int)(blockIdx.y + 1) * FC_SPC);
  const float inv = 1.f / ((float)b * (float)L);
  float mean[2], rstd[2], scale[2], wf[2], k0[2], k1[2];
  for (int f = 0; f < F; ++f) {
    const float* ch = a.chan[j][f];
    mean[f] = ch[c]; rstd[f] = ch[C + c]; scale[f] = ch[2 * C + c];
    wf[f] = w[j * P + a.col[f]];
    k0[f] = training ? a.bn_grad[j][f][C + c] * inv : 0.f;      // dBN.bias / (b L)
    k1[f] = training ? a.bn_grad[j][f][c] * inv : 0.f;          // dBN.weight / (b L)
  }
  float sdu[2] = {0.f, 0.f};
  for (int s = blockIdx.y * FC_SPC + sl.sub; s < s_end; s += sl.nsub) {
    const int64_t e = ((int64_t)s * C + c) * L + sl.l0;
    const float4 g4 = ld4(g + e);
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      if (f < F) {
        const int mish = a.mish[f];
        const int64_t ue = ((int64_t)s * F * C + f * C + c) * L + sl.l0;
        const float4 u4 = ld4(a.U[j] + ue);
        const float4 a4 = act4(u4, mish), d4 = dact4(u4, mish);
        dr.off = dbase + a.doff[j][f];
        const float4 dy = f4_scale(f4_mul(g4, drop_mult4(dr, (uint64_t)e)), wf[f]);
        float4 du;
        du.x = scale[f] * (dy.x - k0[f] - (a4.x - mean[f]) * rstd[f] * k1[f]) * d4.x;
        du.y = scale[f] * (dy.y - k0[f] - (a4.y - mean[f]) * rstd[f] * k1[f]) * d4.y;
        du.z = scale[f] * (dy.z - k0[f] - (a4.z - mean[f]) * rstd[f] * k1[f]) * d4.z;
        du.w = scale[f] * (dy.w - k0[f] - (a4.w - mean[f]) * rstd[f] * k1[f]) * d4.w;
        st4(a.dU[j] + ue, du);
        sdu[f] += f4_hsum(du);
      }
    }
  }
  const bool lead = sl.sub == 0 && sl.l0 == 0;
  for (int f = 0; f < F; ++f) {
    const float t = channel_sum(sdu[f], sl, lgL, red);
    if (lead) atomicAdd(a.dbias[j][f] + c, t);
  }
}

// ------------------------------------------------------------------------------------------ backward GEMMs
struct GemmBwdArgs {
  const float* x[FC_E];
  const float* dU[FC_E];
  const float* W[FC_E][2];
  float* dW[FC_E][2];
  float* dx[FC_E];
  uint32_t qmask[FC_E];
};

constexpr int FC_KCH = 512;      // batch columns per dW block (split-K; the partial tiles meet in dW by atomics)

// 1-D grid: first n_dx * rt * ctl data-gradient blocks (rt row tiles of 64 channels, ctl column tiles of 64), then
// n * F * rt * rt * kch weight-gradient blocks.
__global__ __launch_bounds__(256) void fc_bwd_gemm_k(const GemmBwdArgs a, int n, int F, const float* __restrict__ w,
                                                     int P, uint32_t skip_cols, const float* __restrict__ g, int n_dx,
                                                     int b, int C, int lgL) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lo = lane & 15, h = lane >> 4;
  const int L = 1 << lgL, N = b * L;
  const int rt = (C + 63) / 64, ctl = (N + 63) / 64;
  const int64_t CL = (int64_t)C * L, FCL = (int64_t)F * CL;
  int id = blockIdx.x;
  const int nA = n_dx * rt * ctl;
  f32x4 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (id < nA) {
    // dx[c][col] = sum_{j in qmask} sum_m Wstack_j[m][c] dU_j[m][col] + wskip g:  A = W^T (lane i -> c, slot -> m)
    const int q = id / (rt * ctl);
    id -= q * rt * ctl;
    const int c0 = (id / ctl) * 64 + wave * 16, colbase = (id % ctl) * 64;
    if (c0 >= C) return;
    int64_t cofs[4];
    bool cv[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int col = colbase + ct * 16 + lo;
      cv[ct] = col < N;
      const int cc = cv[ct] ? col : 0;
      cofs[ct] = (int64_t)(cc >> lgL) * FCL + (cc & (L - 1)) + (int64_t)(4 * h) * L;
    }
    float ws = 0.f;
    for (uint32_t mk = a.qmask[q]; mk; mk &= mk - 1) {
      const int j = __ffs(mk) - 1;
      if (skip_cols) ws += skip_weight(w, j, P, skip_cols);
      const float* __restrict__ dU = a.dU[j];
      for (int f = 0; f < F; ++f) {
        const float* wp = a.W[j][f] + (int64_t)(4 * h) * C + c0 + lo;
        for (int k0 = 0; k0 < C; k0 += 16) {
          const float* wq = wp + (int64_t)k0 * C;
          const float a0 = wq[0], a1 = wq[C], a2 = wq[2 * C], a3 = wq[3 * C];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            const float* p = dU + cofs[ct] + (int64_t)(f * C + k0) * L;
            float b0 = p[0], b1 = p[L], b2 = p[2 * L], b3 = p[3 * L];
            if (!cv[ct]) b0 = b1 = b2 = b3 = 0.f;
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b2, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, b3, acc[ct], 0, 0, 0);
          }
        }
      }
    }
    float* __restrict__ dx = a.dx[q];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int col = colbase + ct * 16 + lo;
      if (cv[ct]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t e = (int64_t)(col >> lgL) * CL + (int64_t)(c0 + 4 * h + r) * L + (col & (L - 1));
          dx[e] = acc[ct][r] + (skip_cols ? ws * g[e] : 0.f);
        }
      }
    }
    return;
  }
  // dW_jf[m][k] += sum_col dU_jf[m][col] x_j[k][col]:  A = dU (lane i -> m, slot -> 4 columns), B = x^T
  id -= nA;
  const int kch = (N + FC_KCH - 1) / FC_KCH;
  const int per = rt * rt * kch;
  const int jf = id / per;
  id -= jf * per;
  const int j = jf / F, f = jf - j * F;
  const int mt = id / (rt * kch);
  id -= mt * rt * kch;
  const int kt = id / kch, kc = id - kt * kch;
  const int m0 = mt * 64 + wave * 16;
  if (m0 >= C) return;
  const float* __restrict__ dU = a.dU[j] + (int64_t)(f * C + m0 + lo) * L;
  const float* __restrict__ x = a.x[j];
  int64_t kofs[4];
  bool kv[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int k = kt * 64 + ct * 16 + lo;
    kv[ct] = k < C;
    kofs[ct] = (int64_t)(kv[ct] ? k : 0) * L;
  }
  const int col_end = min(N, (kc + 1) * FC_KCH);
  for (int col0 = kc * FC_KCH; col0 < col_end; col0 += 16) {
    const int col = col0 + 4 * h;
    const bool v = col < col_end;
    const int cc = v ? col : 0;
    const int s = cc >> lgL, l = cc & (L - 1);
    float4 a4 = ld4(dU + (int64_t)s * FCL + l);
    if (!v) a4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      float4 b4 = ld4(x + (int64_t)s * CL + kofs[ct] + l);
      if (!kv[ct]) b4 = make_float4(0.f, 0.f, 0.f, 0.f);
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4.x, acc[ct], 0, 0, 0);
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4.y, acc[ct], 0, 0, 0);
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4.z, acc[ct], 0, 0, 0);
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4.w, acc[ct], 0, 0, 0);
    }
  }
  float* __restrict__ dW = a.dW[j][f];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    if (kv[ct]) {
      const int k = kt * 64 + ct * 16 + lo;
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(dW + (int64_t)(m0 + 4 * h + r) * C + k, acc[ct][r]);
    }
  }
}

// ------------------------------------------------------------------------------------------ found networks
// One output per edge: edge = blockIdx.z, kind / output / incoming gradient / dropout offset per edge.
struct SepFwdArgs {
  const float* U[FC_E];
  float* out[FC_E];
  MixPrim p[FC_E];
  uint64_t doff[FC_E];
  int mish[FC_E];
  DropCfg drop;
};

// grid (C / 16, ceil(b / nsub), edge)
__global__ __launch_bounds__(256) void fc_sep_fwd_k(const SepFwdArgs a, int training, int b, int C, int lgL) {
  const Slab sl = slab_of(lgL);
  const int L = 1 << lgL, j = blockIdx.z;
  DropRt dr = drop_begin(a.drop);
  dr.off += a.doff[j] - a.drop.offset;                 // the step counter plus the edge's own site
  const int s = blockIdx.y * sl.nsub + sl.sub;
  const bool valid = s < b;
  const int sc = valid ? s : 0;
  const int c = sl.c;
  const int64_t e = ((int64_t)sc * C + c) * L + sl.l0;
  const bool writer = blockIdx.y == 0 && sl.sub == 0 && sl.l0 == 0;
  const float nN = (float)b * (float)L;
  const MixPrim& p = a.p[j];
  const int mish = a.mish[j];
  const float4 u4 = ld4(a.U[j] + e);
  float mean, var;
  if (training) {
    const float md = p.stat[c] / nN;
    mean = act_f(p.bias[c], mish) + md;
    var = fmaxf(p.stat[C + c] / nN - md * md, 0.f);
  } else {
    mean = p.rm[c];
    var = p.rv[c];
  }
  const float rstd = rsqrtf(var + FC_EPS);
  const float scale = p.bn_w[c] * rstd, shift = p.bn_b[c] - mean * scale;
  if (writer) {
    p.chan[c] = mean;
    p.chan[C + c] = rstd;
    p.chan[2 * C + c] = scale;
    p.chan[3 * C + c] = shift;
    if (training) {
      p.rm[c] = (1.f - FC_MOMENTUM) * p.rm[c] + FC_MOMENTUM * mean;
      p.rv[c] = (1.f - FC_MOMENTUM) * p.rv[c] + FC_MOMENTUM * var * (nN / (nN - 1.f));
      if (blockIdx.x == 0 && threadIdx.x == 0 && p.nbt != nullptr) p.nbt[0] += 1;
    }
  }
  const float4 a4 = act4(u4, mish);
  const float4 dm = drop_mult4(dr, (uint64_t)e);
  const float4 o = make_float4(dm.x * (scale * a4.x + shift), dm.y * (scale * a4.y + shift),
                               dm.z * (scale * a4.z + shift), dm.w * (scale * a4.w + shift));
  if (valid) st4(a.out[j] + e, o);
}

struct SepBwdArgs {
  const float* U[FC_E];
  const float* g[FC_E];
  float* dU[FC_E];
  const float* chan[FC_E];
  float* bn_grad[FC_E];
  float* dbias[FC_E];
  uint64_t doff[FC_E];
  int mish[FC_E];
  DropCfg drop;
};

// grid (C / 16, ceil(b / FC_SPC), edge)
__global__ __launch_bounds__(256) void fc_sep_bwd_reduce_k(const SepBwdArgs a, int b, int C, int lgL) {
  __shared__ float red[256];
  const Slab sl = slab_of(lgL);
  const int L = 1 << lgL, j = blockIdx.z, c = sl.c;
  DropRt dr = drop_begin(a.drop);
  dr.off += a.doff[j] - a.drop.offset;
  const int s_end = min(b, (int)(blockIdx.y + 1) * FC_SPC);
  const float* __restrict__ ch = a.chan[j];
  const float* __restrict__ g = a.g[j];
  const float* __restrict__ U = a.U[j];
  const float mean = ch[c], rstd = ch[C + c];
  const int mish = a.mish[j];
  float sdy = 0.f, sda = 0.f;
  for (int s = blockIdx.y * FC_SPC + sl.sub; s < s_end; s += sl.nsub) {
    const int64_t e = ((int64_t)s * C + c) * L + sl.l0;
    const float4 g4 = ld4(g + e);
    const float4 a4 = act4(ld4(U + e), mish);
    const float4 gm = f4_mul(g4, drop_mult4(dr, (uint64_t)e));       // dy = mask * g
    const float4 ah = make_float4((a4.x - mean) * rstd, (a4.y - mean) * rstd, (a4.z - mean) * rstd,
                                  (a4.w - mean) * rstd);
    sdy += f4_hsum(gm);
    sda += f4_dot(gm, ah);
  }
  const bool lead = sl.sub == 0 && sl.l0 == 0;
  const float t1 = channel_sum(sda, sl, lgL, red);
  const float t2 = channel_sum(sdy, sl, lgL, red);
  if (lead) {
    atomicAdd(a.bn_grad[j] + c, t1);
    atomicAdd(a.bn_grad[j] + C + c, t2);
  }
}

// grid as fc_sep_bwd_reduce_k
__global__ __launch_bounds__(256) void fc_sep_bwd_du_k(const SepBwdArgs a, int training, int b, int C, int lgL) {
  __shared__ float red[256];
  const Slab sl = slab_of(lgL);
  const int L = 1 << lgL, j = blockIdx.z, c = sl.c;
  DropRt dr = drop_begin(a.drop);
  dr.off += a.doff[j] - a.drop.offset;
  const int s_end = min(b, (int)(blockIdx.y + 1) * FC_SPC);
  const float inv = 1.f / ((float)b * (float)L);
  const float* __restrict__ ch = a.chan[j];
  const float* __restrict__ g = a.g[j];
  const float* __restrict__ U = a.U[j];
  float* __restrict__ dU = a.dU[j];
  const float mean = ch[c], rstd = ch[C + c], scale = ch[2 * C + c];
  const float k0 = training ? a.bn_grad[j][C + c] * inv : 0.f;      // dBN.bias / (b L)
  const float k1 = training ? a.bn_grad[j][c] * inv : 0.f;          // dBN.weight / (b L)
  const int mish = a.mish[j];
  float sdu = 0.f;
  for (int s = blockIdx.y * FC_SPC + sl.sub; s < s_end; s += sl.nsub) {
    const int64_t e = ((int64_t)s * C + c) * L + sl.l0;
    const float4 g4 = ld4(g + e);
    const float4 u4 = ld4(U + e);
    const float4 a4 = act4(u4, mish), d4 = dact4(u4, mish);
    const float4 dy = f4_mul(g4, drop_mult4(dr, (uint64_t)e));
    float4 du;
    du.x = scale * (dy.x - k0 - (a4.x - mean) * rstd * k1) * d4.x;
    du.y = scale * (dy.y - k0 - (a4.y - mean) * rstd * k1) * d4.y;
    du.z = scale * (dy.z - k0 - (a4.z - mean) * rstd * k1) * d4.z;
    du.w = scale * (dy.w - k0 - (a4.w - mean) * rstd * k1) * d4.w;
    st4(dU + e, du);
    sdu += f4_hsum(du);
  }
  const bool lead = sl.sub == 0 && sl.l0 == 0;
  const float t = channel_sum(sdu, sl, lgL, red);
  if (lead) atomicAdd(a.dbias[j] + c, t);
}

int check_common(const bmnas_fc_edge_t* edges, int n, int F, int P, int b, int C, int L) {
  if (!edges || n <= 0 || b <= 0) return BMNAS_E_ARG;
  if (!bmnas_fc_edges_ok(n, F, P, b, C, L)) return (n > FC_E || P > 8) ? BMNAS_E_LIMIT : BMNAS_E_SHAPE;
  for (int j = 0; j < n; ++j) {
    if (!edges[j].x || !edges[j].U) return BMNAS_E_ARG;
    for (int f = 0; f < F; ++f) {
      const bmnas_fc_prim_t& p = edges[j].fc[f];
      if (!p.W || !p.bias || !p.bn_w || !p.bn_b || !p.chan || p.col < 0 || p.col >= P) return BMNAS_E_ARG;
      if (p.mish != edges[0].fc[f].mish || p.col != edges[0].fc[f].col) return BMNAS_E_ARG;
      // one dropout configuration per sum: the sites differ in their offsets only
      if (p.drop.thr != edges[0].fc[0].drop.thr || p.drop.seed != edges[0].fc[0].drop.seed ||
          p.drop.step != edges[0].fc[0].drop.step)
        return BMNAS_E_ARG;
    }
  }
  return 0;
}

DropCfg common_drop(const bmnas_fc_edge_t* edges) {
  DropCfg c = to_cfg(edges[0].fc[0].drop);
  c.offset = 0;
  return c;
}

void fill_bwd(BwdArgs& a, const bmnas_fc_edge_t* edges, int n, int F) {
  a.drop = common_drop(edges);
  for (int f = 0; f < 2; ++f) {
    a.mish[f] = f < F ? edges[0].fc[f].mish : 0;
    a.col[f] = f < F ? edges[0].fc[f].col : 0;
  }
  for (int j = 0; j < n; ++j) {
    a.x[j] = edges[j].x; a.U[j] = edges[j].U; a.dU[j] = edges[j].dU;
    for (int f = 0; f < F; ++f) {
      const bmnas_fc_prim_t& p = edges[j].fc[f];
      a.chan[j][f] = p.chan; a.bn_grad[j][f] = p.bn_grad; a.dbias[j][f] = p.dbias; a.doff[j][f] = p.drop.offset;
    }
  }
}

int lg_of(int L) { return L == 4 ? 2 : (L == 8 ? 3 : 4); }

}  // namespace

extern "C" int bmnas_fc_edges_ok(int n, int F, int P, int b, int C, int L) {
  return n >= 1 && n <= FC_E && (F == 1 || F == 2) && P >= 1 && P <= 8 && b >= 1 && C >= 16 && C % 16 == 0 &&
         (L == 4 || L == 8 || L == 16) && b <= 65535;      // (the sample tiles of the elementwise kernels are grid.y)
}

extern "C" int bmnas_fc_edges_gemm_fwd(const bmnas_fc_edge_t* edges, int n, int F, int training, int b, int C, int L,
                                       void* stream) {
  if (int rc = check_common(edges, n, F, 8, b, C, L)) return rc;
  GemmFwdArgs a = {};
  for (int f = 0; f < F; ++f) a.mish[f] = edges[0].fc[f].mish;
  for (int j = 0; j < n; ++j) {
    a.x[j] = edges[j].x; a.U[j] = edges[j].U;
    for (int f = 0; f < F; ++f) {
      const bmnas_fc_prim_t& p = edges[j].fc[f];
      if (training && !p.stat) return BMNAS_E_ARG;
      a.W[j][f] = p.W; a.bias[j][f] = p.bias; a.stat[j][f] = p.stat;
    }
  }
  const dim3 grid((b * L + 63) / 64, (F * C + 63) / 64, n);
  hipLaunchKernelGGL(fc_gemm_fwd_k, grid, dim3(256), 0, (hipStream_t)stream, a, F, training, b, C, lg_of(L));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_fc_edges_mix_fwd(const bmnas_fc_edge_t* edges, int n, int F, const float* w, int P,
                                      uint32_t skip_cols, int training, float* out, int b, int C, int L,
                                      void* stream) {
  if (int rc = check_common(edges, n, F, P, b, C, L)) return rc;
  if (!w || !out || (skip_cols >> P)) return BMNAS_E_ARG;
  MixArgs a = {};
  a.drop = common_drop(edges);
  for (int f = 0; f < F; ++f) { a.mish[f] = edges[0].fc[f].mish; a.col[f] = edges[0].fc[f].col; }
  for (int j = 0; j < n; ++j) {
    a.x[j] = edges[j].x; a.U[j] = edges[j].U;
    for (int f = 0; f < F; ++f) {
      const bmnas_fc_prim_t& p = edges[j].fc[f];
      if (!p.running_mean || !p.running_var || (training && !p.stat)) return BMNAS_E_ARG;
      a.p[j][f] = MixPrim{p.stat, p.bias, p.bn_w, p.bn_b, p.running_mean, p.running_var,
                          (long long*)p.num_batches_tracked, p.chan};
      a.doff[j][f] = p.drop.offset;
    }
  }
  const int nsub = 256 / (4 * L);
  const dim3 grid(C / 16, (b + nsub - 1) / nsub);
  hipLaunchKernelGGL(fc_mix_fwd_k, grid, dim3(256), 0, (hipStream_t)stream, a, n, F, w, P, skip_cols, training, out, b,
                     C, lg_of(L));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_fc_edges_bwd_reduce(const bmnas_fc_edge_t* edges, int n, int F, const float* w, int P,
                                         uint32_t skip_cols, const float* g, float* dw, int b, int C, int L,
                                         void* stream) {
  if (int rc = check_common(edges, n, F, P, b, C, L)) return rc;
  if (!w || !g || !dw || (skip_cols >> P)) return BMNAS_E_ARG;
  for (int j = 0; j < n; ++j)
    for (int f = 0; f < F; ++f)
      if (!edges[j].fc[f].bn_grad) return BMNAS_E_ARG;
  BwdArgs a = {};
  fill_bwd(a, edges, n, F);
  const dim3 grid(C / 16, (b + FC_SPC - 1) / FC_SPC, n);
  hipLaunchKernelGGL(fc_bwd_reduce_k, grid, dim3(256), 0, (hipStream_t)stream, a, F, w, P, skip_cols, g, dw, b, C,
                     lg_of(L));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_fc_edges_bwd_du(const bmnas_fc_edge_t* edges, int n, int F, const float* w, int P, const float* g,
                                     int training, int b, int C, int L, void* stream) {
  if (int rc = check_common(edges, n, F, P, b, C, L)) return rc;
  if (!w || !g) return BMNAS_E_ARG;
  for (int j = 0; j < n; ++j) {
    if (!edges[j].dU) return BMNAS_E_ARG;
    for (int f = 0; f < F; ++f)
      if (!edges[j].fc[f].bn_grad || !edges[j].fc[f].dbias) return BMNAS_E_ARG;
  }
  BwdArgs a = {};
  fill_bwd(a, edges, n, F);
  const dim3 grid(C / 16, (b + FC_SPC - 1) / FC_SPC, n);
  hipLaunchKernelGGL(fc_bwd_du_k, grid, dim3(256), 0, (hipStream_t)stream, a, F, w, P, g, training, b, C, lg_of(L));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_fc_edges_bwd_gemm(const bmnas_fc_edge_t* edges, int n, int F, const float* w, int P,
                                       uint32_t skip_cols, const float* g, float* const* dxs,
                                       const uint32_t* dx_edges, int n_dx, int b, int C, int L, void* stream) {
  if (int rc = check_common(edges, n, F, P, b, C, L)) return rc;
  if (!w || !g || n_dx < 0 || n_dx > FC_E || (n_dx > 0 && (!dxs || !dx_edges)) || (skip_cols >> P))
    return BMNAS_E_ARG;
  GemmBwdArgs a = {};
  for (int j = 0; j < n; ++j) {
    if (!edges[j].dU) return BMNAS_E_ARG;
    a.x[j] = edges[j].x; a.dU[j] = edges[j].dU;
    for (int f = 0; f < F; ++f) {
      if (!edges[j].fc[f].dW) return BMNAS_E_ARG;
      a.W[j][f] = edges[j].fc[f].W; a.dW[j][f] = edges[j].fc[f].dW;
    }
  }
  for (int q = 0; q < n_dx; ++q) {
    if (!dxs[q] || dx_edges[q] == 0u || (dx_edges[q] >> n)) return BMNAS_E_ARG;
    a.dx[q] = dxs[q]; a.qmask[q] = dx_edges[q];
  }
  const int N = b * L, rt = (C + 63) / 64, ctl = (N + 63) / 64, kch = (N + FC_KCH - 1) / FC_KCH;
  const int64_t blocks = (int64_t)n_dx * rt * ctl + (int64_t)n * F * rt * rt * kch;
  if (blocks > 0x7fffffff) return BMNAS_E_LIMIT;
  hipLaunchKernelGGL(fc_bwd_gemm_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, n, F, w, P, skip_cols,
                     g, n_dx, b, C, lg_of(L));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------ found networks
namespace {

// arguments first, then shape, then limit; the edges' one FC primitive is fc[0]
int check_found(const bmnas_fc_edge_t* edges, int E, int b, int C, int L) {
  if (!edges || E <= 0 || b <= 0) return BMNAS_E_ARG;
  if (!bmnas_fc_edges_ok(E, 1, 1, b, C, L)) return E > FC_E ? BMNAS_E_LIMIT : BMNAS_E_SHAPE;
  for (int j = 0; j < E; ++j) {
    const bmnas_fc_prim_t& p = edges[j].fc[0];
    if (!edges[j].U || !p.chan || (p.mish != 0 && p.mish != 1)) return BMNAS_E_ARG;
    // one dropout configuration per group: the sites differ in their offsets only
    if (p.drop.thr != edges[0].fc[0].drop.thr || p.drop.seed != edges[0].fc[0].drop.seed ||
        p.drop.step != edges[0].fc[0].drop.step)
      return BMNAS_E_ARG;
  }
  return 0;
}

int fill_sep_bwd(SepBwdArgs& a, const bmnas_fc_edge_t* edges, int E, const float* const* gs) {
  if (!gs) return BMNAS_E_ARG;
  a.drop = common_drop(edges);
  for (int j = 0; j < E; ++j) {
    const bmnas_fc_prim_t& p = edges[j].fc[0];
    if (!gs[j] || !p.bn_grad) return BMNAS_E_ARG;
    a.U[j] = edges[j].U; a.g[j] = gs[j]; a.dU[j] = edges[j].dU; a.chan[j] = p.chan; a.bn_grad[j] = p.bn_grad;
    a.dbias[j] = p.dbias; a.doff[j] = p.drop.offset; a.mish[j] = p.mish;
  }
  return 0;
}

}  // namespace

extern "C" int bmnas_fc_found_fwd(const bmnas_fc_edge_t* edges, int E, int training, float* const* outs, int b, int C,
                                  int L, void* stream) {
  if (int rc = check_found(edges, E, b, C, L)) return rc;
  if (!outs) return BMNAS_E_ARG;
  SepFwdArgs a = {};
  a.drop = common_drop(edges);
  for (int j = 0; j < E; ++j) {
    const bmnas_fc_prim_t& p = edges[j].fc[0];
    if (!outs[j] || !p.bias || !p.bn_w || !p.bn_b || !p.running_mean || !p.running_var || (training && !p.stat))
      return BMNAS_E_ARG;
    a.U[j] = edges[j].U; a.out[j] = outs[j];
    a.p[j] = MixPrim{p.stat, p.bias, p.bn_w, p.bn_b, p.running_mean, p.running_var,
                     (long long*)p.num_batches_tracked, p.chan};
    a.doff[j] = p.drop.offset; a.mish[j] = p.mish;
  }
  const int nsub = 256 / (4 * L);
  const dim3 grid(C / 16, (b + nsub - 1) / nsub, E);
  hipLaunchKernelGGL(fc_sep_fwd_k, grid, dim3(256), 0, (hipStream_t)stream, a, training, b, C, lg_of(L));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_fc_found_bwd_reduce(const bmnas_fc_edge_t* edges, int E, const float* const* gs, int b, int C,
                                         int L, void* stream) {
  if (int rc = check_found(edges, E, b, C, L)) return rc;
  SepBwdArgs a = {};
  if (int rc = fill_sep_bwd(a, edges, E, gs)) return rc;
  const dim3 grid(C / 16, (b + FC_SPC - 1) / FC_SPC, E);
  hipLaunchKernelGGL(fc_sep_bwd_reduce_k, grid, dim3(256), 0, (hipStream_t)stream, a, b, C, lg_of(L));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_fc_found_bwd_du(const bmnas_fc_edge_t* edges, int E, const float* const* gs, int training, int b,
                                     int C, int L, void* stream) {
  if (int rc = check_found(edges, E, b, C, L)) return rc;
  SepBwdArgs a = {};
  if (int rc = fill_sep_bwd(a, edges, E, gs)) return rc;
  for (int j = 0; j < E; ++j)
    if (!edges[j].dU || !edges[j].fc[0].dbias) return BMNAS_E_ARG;
  const dim3 grid(C / 16, (b + FC_SPC - 1) / FC_SPC, E);
  hipLaunchKernelGGL(fc_sep_bwd_du_k, grid, dim3(256), 0, (hipStream_t)stream, a, training, b, C, lg_of(L));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

// fc_bwd_gemm_k is kind-agnostic: one launch for edges of both kinds (F = 1, no skip term, no weight row)
extern "C" int bmnas_fc_found_bwd_gemm(const bmnas_fc_edge_t* edges, int E, float* const* dxs,
                                       const uint32_t* dx_edges, int n_dx, int b, int C, int L, void* stream) {
  if (!edges || E <= 0 || b <= 0 || n_dx < 0 || n_dx > FC_E || (n_dx > 0 && (!dxs || !dx_edges))) return BMNAS_E_ARG;
  if (!bmnas_fc_edges_ok(E, 1, 1, b, C, L)) return E > FC_E ? BMNAS_E_LIMIT : BMNAS_E_SHAPE;
  GemmBwdArgs a = {};
  for (int j = 0; j < E; ++j) {
    if (!edges[j].x || !edges[j].dU || !edges[j].fc[0].W || !edges[j].fc[0].dW) return BMNAS_E_ARG;
    a.x[j] = edges[j].x; a.dU[j] = edges[j].dU; a.W[j][0] = edges[j].fc[0].W; a.dW[j][0] = edges[j].fc[0].dW;
  }
  for (int q = 0; q < n_dx; ++q) {
    if (!dxs[q] || dx_edges[q] == 0u || (dx_edges[q] >> E)) return BMNAS_E_ARG;
    a.dx[q] = dxs[q]; a.qmask[q] = dx_edges[q];
  }
  const int N = b * L, rt = (C + 63) / 64, ctl = (N + 63) / 64, kch = (N + FC_KCH - 1) / FC_KCH;
  const int64_t blocks = (int64_t)n_dx * rt * ctl + (int64_t)E * rt * rt * kch;
  if (blocks > 0x7fffffff) return BMNAS_E_LIMIT;
  hipLaunchKernelGGL(fc_bwd_gemm_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, E, 1,
                     (const float*)nullptr, 1, 0u, (const float*)nullptr, n_dx, b, C, lg_of(L));
  BMNAS_CHECK_LAUNCH();
  return 0;
}
