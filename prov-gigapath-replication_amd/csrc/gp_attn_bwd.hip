// Attention backward at the flash_attn_func seam for gfx950: (dq, dk, dv) = f(q, k, v, o, lse, dout),
// non-causal, no mask, dropout 0.  Replaces flash-attn's CUDA backward behind flash_attn_func
// (torchscale/component/flash_attention.py:13-16); the LSE carries no gradient, as in
// DilatedAttention.scattering (dilated_attention.py:119-124, torch.no_grad()).
//
// Store-and-own, two launches, no atomics, no inter-workgroup waits (bitwise reproducible):
//   1. attn_bwd_dq_kernel: a workgroup owns 128 query rows of one (batch, head) and loops over the keys in
//      LDS tiles of 64.  It also computes delta_i = sum_d dO_id O_id for its rows (with the MFMA sequence of
//      dP, so that dP - delta cancels exactly where it should) and stores it for the second launch.
//        S^T = K.Q^T, dP^T = V.dO^T      (row-wise LDS reads of K / V; Q / dO fragments live in registers)
//        dS^T = P^T o (dP^T - delta)      P^T = exp(c S^T - lse), recomputed, fp32
//        dQ^T += K^T.dS^T                 (K^T fragments by transposed LDS reads of the same K image)
//   2. attn_bwd_dkv_kernel: a workgroup owns 128 keys and loops over the queries in LDS tiles of 64
//      (Q, dO, lse, delta).
//        S = Q.K^T, dP = dO.V^T           (row-wise LDS reads of Q / dO; K / V fragments live in registers)
//        dV^T += dO^T.P, dK^T += Q^T.dS   (transposed LDS reads of the same dO / Q images)
// All products are v_mfma_f32_16x16x32 (D = 48 pads the second d step of S and dP with zeros), fp32
// accumulation; P and dS are rounded to the 16-bit format only as MFMA operands; results are rounded once,
// on store.  Tails by predication: rows past seqlen are loaded as zeros and never stored, a tail key gets
// P = 0 by a select, a tail query gets lse = +inf.  This file is compiled with NaNs honoured: a non-finite
// dout reaches all three gradients.
#include <math.h>

#include "gp_api.h"
#include "gp_common.h"

namespace {

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kWaves = 4;
constexpr int kSub = 2;                        // 16-row sub-tiles a wave owns
constexpr int kOwn = kWaves * kSub * 16;       // 128 rows (queries or keys) a workgroup owns
constexpr int kTile = 64;                      // rows of a streamed LDS tile
constexpr float kLog2e = 1.4426950408889634f;

template <bool kH>
GP_DEV f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 c) {     // 16x16 += [16 x 32].[32 x 16]
  if constexpr (kH)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <bool kH>
GP_DEV __bf16 f2e_slot(float f) { return __builtin_bit_cast(__bf16, f2e<kH>(f)); }

// Blocks b, b + 8, ... share an XCD: give each XCD runs of 8 consecutive work items (tiles of one
// (batch, head)), which stream the same rows through that XCD's L2 (as gp_attn.hip's xcd_group).
GP_DEV int64_t xcd_group(int64_t bid, int64_t nb) {
  constexpr int64_t G = 8, C = 8 * G;
  const int64_t full = nb - nb % C;
  if (bid >= full) return bid;
  const int64_t base = bid - bid % C;
  const int64_t in = bid % C;
  return base + (in & 7) * G + (in >> 3);
}

struct BwdArgs {
  const uint16_t *q, *k, *v, *o, *dout;
  const float* lse;
  float* delta;          // [nbatch, H, L] fp32 (workspace)
  uint16_t *dq, *dk, *dv;
  int32_t L, H;
  int32_t ntile;         // ceil(L / kOwn)
  float c, c_log2;       // softmax_scale, softmax_scale * log2(e)
};

// Fragments of one 16-row sub-tile for the products that contract over d: lane (l16, g4) holds row l16,
// d = 32 ks + 8 g4 .. + 7 of k-step ks; D = 48 pads its second step with zeros (lanes g4 >= 2 load nothing).
// Every step is the same v_mfma_f32_16x16x32: a 16x16x16 step for d = 32..47 chained onto the 16x16x32 result
// with no instruction between them returned wrong sums on the MI355X.
template <int D>
struct RowFrag {
  static constexpr int KS = (D + 31) / 32;
  bf16x8 f[KS];
};
template <int D, typename P>
GP_DEV void load_rowfrag(RowFrag<D>& r, P row, int g4, bool valid) {   // row: 16-byte aligned, D elements
#pragma unroll
  for (int ks = 0; ks < RowFrag<D>::KS; ++ks) {
    bf16x8 z = {};
    if (valid && ks * 32 + g4 * 8 < D) z = *reinterpret_cast<const bf16x8*>(row + ks * 64 + g4 * 16);
    r.f[ks] = z;
  }
}
template <int D, bool kH>
GP_DEV f32x4 dot_rows(const RowFrag<D>& a, const RowFrag<D>& b, f32x4 acc) {   // acc[m][n] += a_m . b_n
#pragma unroll
  for (int ks = 0; ks < RowFrag<D>::KS; ++ks) acc = mfma32<kH>(a.f[ks], b.f[ks], acc);
  return acc;
}

// A operand X^T[d 16 dt + l16][row] of a product that contracts over 32 tile rows, from the row-major
// LDS image of X by two transposed reads: element e < 4 is tile row r32 + 4 g4 + e, e >= 4 is
// r32 + 16 + 4 g4 + e - 4 -- the order in which two C-layout sub-tiles (rows 4 g4 + reg) pack into
// the B operand.
template <int ROWB>
GP_DEV bf16x8 read_transposed(const char* img, int r32, int dt, int l16, int g4) {
  const char* base = img + (r32 + 4 * g4 + (l16 >> 2)) * ROWB + (16 * dt + 4 * (l16 & 3)) * 2;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + 16 * ROWB));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// Streams two [kTile x D] row-major tiles (rows past L as zeros) global -> registers -> LDS.
template <int D>
struct TileStage {
  static constexpr int ROWB = 2 * D + 16;     // +16: the 16-row ds_read_b128 fragment reads spread over all banks
  static constexpr int TILEB = kTile * ROWB;
  static constexpr int CH = D / 8;            // 16-byte chunks per row
  static constexpr int LPT = 2 * kTile * CH / 256;
  static_assert((2 * kTile * CH) % 256 == 0, "two tiles must split evenly over 256 threads");
  uint4 r[LPT];
  GP_DEV void load(const uint16_t* x0, const uint16_t* x1, int64_t rs, int row0, int L) {
#pragma unroll
    for (int u = 0; u < LPT; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int tsel = idx / (kTile * CH);
      const int rem = idx % (kTile * CH);
      const int row = rem / CH, ch = rem % CH;
      uint4 z = make_uint4(0, 0, 0, 0);
      if (row0 + row < L) z = *reinterpret_cast<const uint4*>((tsel ? x1 : x0) + (int64_t)(row0 + row) * rs + ch * 8);
      r[u] = z;
    }
  }
  GP_DEV void store(char* buf) const {         // buf: [tile 0 | tile 1]
#pragma unroll
    for (int u = 0; u < LPT; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int tsel = idx / (kTile * CH);
      const int rem = idx % (kTile * CH);
      const int row = rem / CH, ch = rem % CH;
      *reinterpret_cast<uint4*>(buf + tsel * TILEB + row * ROWB + ch * 16) = r[u];
    }
  }
};

// ---------------------------------------------------------------------------------------
// dQ (and delta): one workgroup per 128 query rows of a (batch, head).
template <int D, bool kH>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const BwdArgs a) {
  using TS = TileStage<D>;
  constexpr int DT = D / 16, ROWB = TS::ROWB, TILEB = TS::TILEB;
  __shared__ __attribute__((aligned(16))) char smem[4 * TILEB];   // [K0 | V0 | K1 | V1]

  const int64_t item = xcd_group(blockIdx.x, gridDim.x);
  const int tile = (int)(item % a.ntile);
  const int64_t bh = item / a.ntile;
  const int b = (int)(bh / a.H), h = (int)(bh % a.H);
  const int L = a.L;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int64_t rs = (int64_t)a.H * D;
  const int64_t base = ((int64_t)b * L * a.H + h) * D;
  const uint16_t* kb = a.k + base;
  const uint16_t* vb = a.v + base;
  const int q0 = tile * kOwn + w * (kSub * 16);

  // Q / dO fragments (B operands: column = query l16), delta and lse of the wave's rows
  RowFrag<D> qf[kSub], dof[kSub];
  float lse2[kSub], dl[kSub];
#pragma unroll
  for (int qt = 0; qt < kSub; ++qt) {
    const int i = q0 + qt * 16 + l16;
    const bool valid = i < L;
    const int64_t off = base + (int64_t)i * rs;
    load_rowfrag<D>(qf[qt], reinterpret_cast<const char*>(a.q + off), g4, valid);
    load_rowfrag<D>(dof[qt], reinterpret_cast<const char*>(a.dout + off), g4, valid);
    RowFrag<D> of;
    load_rowfrag<D>(of, reinterpret_cast<const char*>(a.o + off), g4, valid);
    // delta: the diagonal of O.dO^T, summed exactly as dP sums dO.V^T
    const f32x4 dd = dot_rows<D, kH>(of, dof[qt], f32x4{0.f, 0.f, 0.f, 0.f});
    const int r = l16 & 3;
    const float pick = r == 0 ? dd[0] : r == 1 ? dd[1] : r == 2 ? dd[2] : dd[3];   // lane g4 == l16 / 4 holds it
    dl[qt] = __shfl(pick, ((l16 >> 2) << 4) | l16, 64);
    lse2[qt] = valid ? a.lse[bh * L + i] * kLog2e : INFINITY;
    if (valid && g4 == 0) a.delta[bh * L + i] = dl[qt];
  }

  f32x4 acc[kSub][DT];
#pragma unroll
  for (int qt = 0; qt < kSub; ++qt)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  TS st;
  const int ntiles = (L + kTile - 1) / kTile;
  st.load(kb, vb, rs, 0, L);
  st.store(smem);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int kv0 = t * kTile;
    if (t + 1 < ntiles) st.load(kb, vb, rs, kv0 + kTile, L);
    const char* Kb = smem + (2 * (t & 1)) * TILEB;
    const char* Vb = Kb + TILEB;
    const bool tail = kv0 + kTile > L;
#pragma unroll
    for (int u = 0; u < kTile / 32; ++u) {
      // S^T / dP^T [key][q] of two 16-key sub-tiles: lane holds keys 32u + 16kt + 4g4 + reg of query l16
      f32x4 sacc[kSub][2], dpacc[kSub][2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        RowFrag<D> kk, vv;
        load_rowfrag<D>(kk, Kb + (32 * u + 16 * kt + l16) * ROWB, g4, true);
        load_rowfrag<D>(vv, Vb + (32 * u + 16 * kt + l16) * ROWB, g4, true);
#pragma unroll
        for (int qt = 0; qt < kSub; ++qt) {
          sacc[qt][kt] = dot_rows<D, kH>(kk, qf[qt], f32x4{0.f, 0.f, 0.f, 0.f});
          dpacc[qt][kt] = dot_rows<D, kH>(vv, dof[qt], f32x4{0.f, 0.f, 0.f, 0.f});
        }
      }
      bf16x8 dsf[kSub];
#pragma unroll
      for (int qt = 0; qt < kSub; ++qt)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float p = __builtin_amdgcn_exp2f(fmaf(sacc[qt][kt][r], a.c_log2, -lse2[qt]));
            if (tail) p = (kv0 + 32 * u + 16 * kt + 4 * g4 + r < L) ? p : 0.f;
            dsf[qt][4 * kt + r] = f2e_slot<kH>(p * (dpacc[qt][kt][r] - dl[qt]));
          }
      // dQ^T[d][q] += K^T[d][key] . dS^T[key][q]
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 kT = read_transposed<ROWB>(Kb, 32 * u, dt, l16, g4);
#pragma unroll
        for (int qt = 0; qt < kSub; ++qt) acc[qt][dt] = mfma32<kH>(kT, dsf[qt], acc[qt][dt]);
      }
    }
    if (t + 1 < ntiles) st.store(smem + (2 * ((t + 1) & 1)) * TILEB);
    __syncthreads();
  }

#pragma unroll
  for (int qt = 0; qt < kSub; ++qt) {
    const int i = q0 + qt * 16 + l16;
    if (i < L) {
      uint16_t* row = a.dq + base + (int64_t)i * rs;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const float vv[4] = {acc[qt][dt][0] * a.c, acc[qt][dt][1] * a.c, acc[qt][dt][2] * a.c, acc[qt][dt][3] * a.c};
        store_e<kH, 4>(row + 16 * dt + 4 * g4, vv);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// dK / dV: one workgroup per 128 keys of a (batch, head).
template <int D, bool kH>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const BwdArgs a) {
  using TS = TileStage<D>;
  constexpr int DT = D / 16, ROWB = TS::ROWB, TILEB = TS::TILEB;
  constexpr int STATB = 2 * kTile * 4;                            // lse * log2(e) | delta of a query tile
  __shared__ __attribute__((aligned(16))) char smem[4 * TILEB + 2 * STATB];   // [Q0 | dO0 | Q1 | dO1 | stat0 | stat1]

  const int64_t item = xcd_group(blockIdx.x, gridDim.x);
  const int tile = (int)(item % a.ntile);
  const int64_t bh = item / a.ntile;
  const int b = (int)(bh / a.H), h = (int)(bh % a.H);
  const int L = a.L;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int64_t rs = (int64_t)a.H * D;
  const int64_t base = ((int64_t)b * L * a.H + h) * D;
  const uint16_t* qb = a.q + base;
  const uint16_t* dob = a.dout + base;
  const float* lseb = a.lse + bh * L;
  const float* delb = a.delta + bh * L;
  const int k0 = tile * kOwn + w * (kSub * 16);

  // K / V fragments (B operands: column = key l16) of the wave's keys
  RowFrag<D> kf[kSub], vf[kSub];
#pragma unroll
  for (int kt = 0; kt < kSub; ++kt) {
    const int key = k0 + kt * 16 + l16;
    const int64_t off = base + (int64_t)key * rs;
    load_rowfrag<D>(kf[kt], reinterpret_cast<const char*>(a.k + off), g4, key < L);
    load_rowfrag<D>(vf[kt], reinterpret_cast<const char*>(a.v + off), g4, key < L);
  }

  f32x4 dkacc[kSub][DT], dvacc[kSub][DT];
#pragma unroll
  for (int kt = 0; kt < kSub; ++kt)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      dkacc[kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dvacc[kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  TS st;
  float sv = 0.f;   // threads 0..63: lse * log2(e) (+inf past L), 64..127: delta (0 past L) of tile row tid & 63
  auto load_stat = [&](int row0) {
    if (threadIdx.x < 2 * kTile) {
      const int i = row0 + (threadIdx.x & (kTile - 1));
      if (threadIdx.x < kTile) sv = i < L ? lseb[i] * kLog2e : INFINITY;
      else sv = i < L ? delb[i] : 0.f;
    }
  };
  auto store_stat = [&](int buf) {
    if (threadIdx.x < 2 * kTile) reinterpret_cast<float*>(smem + 4 * TILEB + buf * STATB)[threadIdx.x] = sv;
  };

  const int ntiles = (L + kTile - 1) / kTile;
  st.load(qb, dob, rs, 0, L);
  load_stat(0);
  st.store(smem);
  store_stat(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) {
      st.load(qb, dob, rs, (t + 1) * kTile, L);
      load_stat((t + 1) * kTile);
    }
    const char* Qb = smem + (2 * (t & 1)) * TILEB;
    const char* Ob = Qb + TILEB;
    const float* stat = reinterpret_cast<const float*>(smem + 4 * TILEB + (t & 1) * STATB);
#pragma unroll
    for (int u = 0; u < kTile / 32; ++u) {
      // S / dP [q][key] of two 16-query sub-tiles: lane holds queries 32u + 16qs + 4g4 + reg of key l16
      f32x4 sacc[2][kSub], dpacc[2][kSub];
#pragma unroll
      for (int qs = 0; qs < 2; ++qs) {
        RowFrag<D> qq, dd;
        load_rowfrag<D>(qq, Qb + (32 * u + 16 * qs + l16) * ROWB, g4, true);
        load_rowfrag<D>(dd, Ob + (32 * u + 16 * qs + l16) * ROWB, g4, true);
#pragma unroll
        for (int kt = 0; kt < kSub; ++kt) {
          sacc[qs][kt] = dot_rows<D, kH>(qq, kf[kt], f32x4{0.f, 0.f, 0.f, 0.f});
          dpacc[qs][kt] = dot_rows<D, kH>(dd, vf[kt], f32x4{0.f, 0.f, 0.f, 0.f});
        }
      }
      bf16x8 pf[kSub], dsf[kSub];
#pragma unroll
      for (int qs = 0; qs < 2; ++qs) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(stat + 32 * u + 16 * qs + 4 * g4);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(stat + kTile + 32 * u + 16 * qs + 4 * g4);
#pragma unroll
        for (int kt = 0; kt < kSub; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(fmaf(sacc[qs][kt][r], a.c_log2, -l4[r]));   // tail query: exp2(-inf) = 0
            pf[kt][4 * qs + r] = f2e_slot<kH>(p);
            dsf[kt][4 * qs + r] = f2e_slot<kH>(p * (dpacc[qs][kt][r] - d4[r]));
          }
      }
      // dV^T[d][key] += dO^T[d][q] . P[q][key];  dK^T[d][key] += Q^T[d][q] . dS[q][key]
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 oT = read_transposed<ROWB>(Ob, 32 * u, dt, l16, g4);
        const bf16x8 qT = read_transposed<ROWB>(Qb, 32 * u, dt, l16, g4);
#pragma unroll
        for (int kt = 0; kt < kSub; ++kt) {
          dvacc[kt][dt] = mfma32<kH>(oT, pf[kt], dvacc[kt][dt]);
          dkacc[kt][dt] = mfma32<kH>(qT, dsf[kt], dkacc[kt][dt]);
        }
      }
    }
    if (t + 1 < ntiles) {
      st.store(smem + (2 * ((t + 1) & 1)) * TILEB);
      store_stat((t + 1) & 1);
    }
    __syncthreads();
  }

#pragma unroll
  for (int kt = 0; kt < kSub; ++kt) {
    const int key = k0 + kt * 16 + l16;
    if (key < L) {
      const int64_t off = base + (int64_t)key * rs;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const float kk[4] = {dkacc[kt][dt][0] * a.c, dkacc[kt][dt][1] * a.c, dkacc[kt][dt][2] * a.c, dkacc[kt][dt][3] * a.c};
        const float vv[4] = {dvacc[kt][dt][0], dvacc[kt][dt][1], dvacc[kt][dt][2], dvacc[kt][dt][3]};
        store_e<kH, 4>(a.dk + off + 16 * dt + 4 * g4, kk);
        store_e<kH, 4>(a.dv + off + 16 * dt + 4 * g4, vv);
      }
    }
  }
}

template <int D, bool kH>
void launch_bwd(const BwdArgs& a, unsigned grid, hipStream_t s) {
  attn_bwd_dq_kernel<D, kH><<<grid, 256, 0, s>>>(a);
  attn_bwd_dkv_kernel<D, kH><<<grid, 256, 0, s>>>(a);
}

bool bwd_dim_ok(int D) { return D == 48 || D == 64 || D == 96; }

}  // namespace

extern "C" size_t gp_seg_attn_bwd_workspace_bytes(int64_t nbatch, int64_t seqlen, int H, int D) {
  if (nbatch <= 0 || seqlen <= 0 || seqlen >= (int64_t)0x7fffffff || H <= 0 || !bwd_dim_ok(D)) return 0;
  const uint64_t n = (uint64_t)nbatch * (uint64_t)H * (uint64_t)seqlen * sizeof(float);   // delta
  return (size_t)((n + 255) / 256 * 256);
}

extern "C" int gp_seg_attn_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* o,
                               const float* lse, const uint16_t* dout, int64_t nbatch, int64_t seqlen, int H, int D,
                               float softmax_scale, uint16_t* dq, uint16_t* dk, uint16_t* dv, void* workspace,
                               size_t workspace_bytes, int fmt, void* stream) {
  GP_REQUIRE(bwd_dim_ok(D), "gp_seg_attn_bwd: head dim %d unsupported (D in {48, 64, 96})", D);
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16, "gp_seg_attn_bwd: bad fmt %d (GP_FMT_BF16 or GP_FMT_F16)", fmt);
  const void* ptrs[] = {q, k, v, o, lse, dout, dq, dk, dv};
  const char* names[] = {"q", "k", "v", "o", "lse", "dout", "dq", "dk", "dv"};
  for (int i = 0; i < 9; ++i) {
    GP_REQUIRE(ptrs[i] != nullptr, "gp_seg_attn_bwd: null pointer (%s)", names[i]);
    GP_REQUIRE(gp_aligned(ptrs[i], i == 4 ? 4 : 16), "gp_seg_attn_bwd: misaligned pointer (%s)", names[i]);
  }
  GP_REQUIRE(seqlen > 0 && seqlen < (int64_t)0x7fffffff, "gp_seg_attn_bwd: bad seqlen %lld", (long long)seqlen);
  GP_REQUIRE(nbatch > 0 && H > 0, "gp_seg_attn_bwd: bad nbatch %lld / H %d", (long long)nbatch, H);
  const size_t need = gp_seg_attn_bwd_workspace_bytes(nbatch, seqlen, H, D);
  GP_REQUIRE(workspace != nullptr && workspace_bytes >= need,
             "gp_seg_attn_bwd: workspace too small (%zu bytes, gp_seg_attn_bwd_workspace_bytes asks %zu)",
             workspace ? workspace_bytes : (size_t)0, need);
  GP_REQUIRE(gp_aligned(workspace, 16), "gp_seg_attn_bwd: misaligned workspace (16 bytes)");
  const int64_t ntile = (seqlen + kOwn - 1) / kOwn;
  const int64_t grid = nbatch * H * ntile;
  GP_REQUIRE(grid < (int64_t)0x7fffffff, "gp_seg_attn_bwd: %lld work items exceed one launch", (long long)grid);

  BwdArgs a;
  a.q = q; a.k = k; a.v = v; a.o = o; a.dout = dout; a.lse = lse;
  a.delta = static_cast<float*>(workspace);
  a.dq = dq; a.dk = dk; a.dv = dv;
  a.L = (int32_t)seqlen; a.H = H; a.ntile = (int32_t)ntile;
  a.c = softmax_scale != 0.f ? softmax_scale : 1.0f / sqrtf((float)D);
  a.c_log2 = a.c * kLog2e;
  hipStream_t s = gp_stream(stream);
  const bool kh = fmt == GP_FMT_F16;
  switch (D) {
    case 48: if (kh) launch_bwd<48, true>(a, (unsigned)grid, s); else launch_bwd<48, false>(a, (unsigned)grid, s); break;
    case 64: if (kh) launch_bwd<64, true>(a, (unsigned)grid, s); else launch_bwd<64, false>(a, (unsigned)grid, s); break;
    default: if (kh) launch_bwd<96, true>(a, (unsigned)grid, s); else launch_bwd<96, false>(a, (unsigned)grid, s); break;
  }
  return gp_check_launch("gp_seg_attn_bwd");
}
