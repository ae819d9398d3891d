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
//
// The same two kernels, templated over the addressing (kDil), are the backward of the fused dilated attention
// (gp_dilated_attn_bwd: gp_dilated_attn_fwd + the no-LN gp_branch_merge_ln; DilatedAttention.forward,
// dilated_attention.py:133-211).  There a work item is (segment, head, 128-row tile) of one branch and the dilated
// gather is folded into the addressing, as in the forward: sparse row i of segment n and head h (phase
// j = h / hpg) reads q / k / v at token n s + i r + j (row stride r * row_stride; a zero pad where i r + j >= s or
// the token >= L) and its dout / lse / delta at row i of the branch's own [B nseg, m, H, D] / [B nseg, H, m]
// buffers.  Three row counts replace seqlen: nk valid keys (= rows with a real q), nq rows that carry a dout
// (merge slot n g + i r + j < L: exactly the rows the forward wrote), min(nk, nq) rows whose dq is stored.
// merge_bwd_kernel writes dout_b = w_b dmerged first; the branches then run in order and add into
// fp32 accumulators (a (token, head) belongs to one sparse row per branch: plain read-add-write, no atomics),
// which grad_store_kernel rounds once.
//
// A third addressing (VarArgs) runs the same kernels over slides packed token-major in one qkv buffer
// (gp_dilated_attn_bwd_varlen): a work item of a branch is (slide, segment, head, 128-row tile), decoded through a
// per-branch table of one VarEntry per slide in device memory -- the slide by a search of the wave-uniform prefix of
// item counts, its entry by scalar loads.  Each slide keeps the geometry of its own length: nk / nq / npad come from
// L_i, never from the packed row count, so the row after a slide's last token (the next slide's CLS) is a tail row
// like any other.  Everything after make_view is the source the other two instantiations compile.
#include <math.h>

#include <cstring>

#include <type_traits>

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

// One branch of gp_dilated_attn_bwd (kDil): dense q / k / v rows, the branch's own dout / lse / delta buffers.
struct DilArgs {
  const uint16_t *q, *k, *v;     // [B*L, row_stride], head h at columns h*D
  const uint16_t *o, *dout;      // [B*nseg, m, H, D]: the forward's o_b; w_b * dmerged (merge_bwd_kernel)
  const float* lse;              // [B*nseg, H, m]
  float* delta;                  // [B*nseg, H, m] fp32 (workspace)
  float *gq, *gk, *gv;           // fp32 accumulators [B*L, H*D]
  int64_t row_stride, L;
  GpBranch g;
  int32_t H;
  int32_t ntile;                 // ceil(m / kOwn)
  float c, c_log2;               // factor of dq / dk; factor of q.k in the log2-domain logit
};

// One slide of one branch of gp_dilated_attn_bwd_varlen (device table, [nbranch][nslide]).
struct VarEntry {
  GpBranch g;                    // the branch's geometry for this slide's L
  int32_t ntile;                 // ceil(g.m / kOwn)
  int32_t item_begin;            // exclusive prefix of nseg * H * ntile over the branch's slides
  int64_t L;                     // the slide's length (CLS + tiles)
  int64_t tok0;                  // its first packed row (tok_off)
  int64_t o_off, lse_off;        // elements: its region in the branch's packed o / dout and lse / delta buffers
};
static_assert(sizeof(VarEntry) == 64, "VarEntry is read as 16 words");

// One branch of gp_dilated_attn_bwd_varlen: the packed q / k / v rows and the branch's packed buffers.
struct VarArgs {
  const uint16_t *q, *k, *v;     // [T, row_stride], head h at columns h*D
  const uint16_t *o, *dout;      // slide-major regions [nseg_i, m_i, H, D]
  const float* lse;              // slide-major regions [nseg_i, H, m_i]
  float* delta;
  float *gq, *gk, *gv;           // fp32 accumulators [T, H*D]
  int64_t row_stride;
  const VarEntry* tab;           // this branch's nslide entries
  int32_t nslide, H;
  float c, c_log2;
};

// What one work item (a (batch, head) of the seam, a (segment, head) of a dilated branch) addresses.
struct View {
  const uint16_t *q, *k, *v, *dout, *o;
  const float* lse;
  float* delta;
  uint16_t *dq, *dk, *dv;        // seam: 16-bit results, row stride rs
  float *gq, *gk, *gv;           // dilated: fp32 accumulators, row stride grs
  int64_t rs, rso, grs;          // row strides of q / k / v, of o / dout, of the accumulators
  int nk, nq;                    // valid keys (= rows with a real q); query rows that carry a dout
  int npad;                      // zero-pad keys in the saved LSE (score 0, v = 0): m - nk; the seam has none
};

// make_view: the item's View; returns its 128-row tile.
template <int D>
GP_DEV int make_view(const BwdArgs& a, int64_t item, View& w) {
  const int tile = (int)(item % a.ntile);
  const int64_t bh = item / a.ntile;
  const int b = (int)(bh / a.H), h = (int)(bh % a.H);
  const int64_t base = ((int64_t)b * a.L * a.H + h) * D;
  w.q = a.q + base; w.k = a.k + base; w.v = a.v + base; w.dout = a.dout + base; w.o = a.o + base;
  w.lse = a.lse + bh * a.L;
  w.delta = a.delta + bh * a.L;
  w.dq = a.dq + base; w.dk = a.dk + base; w.dv = a.dv + base;
  w.gq = w.gk = w.gv = nullptr;
  w.rs = w.rso = (int64_t)a.H * D;
  w.grs = 0;
  w.nk = w.nq = a.L;
  w.npad = 0;
  return tile;
}
// Segment n, head h of a sequence of L tokens whose token 0 is packed row row0 and whose o / dout and lse / delta
// regions start at obase / sbase (elements) of the branch's buffers.  L is the sequence's own length: every row
// limit below is taken against it.
template <int D, class A>
GP_DEV void dil_view(const A& a, const GpBranch& g, int64_t L, int64_t row0, int64_t obase, int64_t sbase, int n, int h,
                     View& w) {
  const int j = h / g.hpg;
  const int64_t tok0 = row0 + (int64_t)n * g.s + j;                      // the token of sparse row 0
  const int64_t off = tok0 * a.row_stride + h * D;
  w.q = a.q + off; w.k = a.k + off; w.v = a.v + off;
  const int64_t ooff = obase + ((int64_t)n * g.m * a.H + h) * D;
  w.dout = a.dout + ooff;
  w.o = a.o + ooff;
  const int64_t soff = sbase + ((int64_t)n * a.H + h) * g.m;
  w.lse = a.lse + soff;
  w.delta = a.delta + soff;
  w.dq = w.dk = w.dv = nullptr;
  const int64_t goff = tok0 * ((int64_t)a.H * D) + h * D;
  w.gq = a.gq + goff; w.gk = a.gk + goff; w.gv = a.gv + goff;
  w.rs = a.row_stride * g.r;
  w.rso = (int64_t)a.H * D;
  w.grs = (int64_t)a.H * D * g.r;
  w.nk = gp_valid_rows(g, L, n, j);
  const int64_t lim = L - ((int64_t)n * g.g + j);                        // merge slots n g + i r + j < L
  const int64_t nq = lim > 0 ? (lim + g.r - 1) / g.r : 0;
  w.nq = (int)(nq < g.m ? nq : g.m);
  w.npad = g.m - w.nk;
}
template <int D>
GP_DEV int make_view(const DilArgs& a, int64_t item, View& w) {
  const GpBranch& g = a.g;
  const int tile = (int)(item % a.ntile);
  const int64_t bh = item / a.ntile;
  const int bn = (int)(bh / a.H), h = (int)(bh % a.H);
  const int bidx = bn / g.nseg, n = bn % g.nseg;
  const int64_t seg0 = (int64_t)bidx * g.nseg;
  dil_view<D>(a, g, a.L, (int64_t)bidx * a.L, seg0 * g.m * a.H * D, seg0 * a.H * g.m, n, h, w);
  return tile;
}

// A table entry by scalar loads (wave-uniform address, constant address space) instead of flat loads into VGPRs,
// as the forward's varlen decode does.
GP_DEV void load_entry_scalar(const VarEntry* src_entry, VarEntry& e) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t words[sizeof(VarEntry) / 4];
  const __attribute__((address_space(4))) uint32_t* src =
      (const __attribute__((address_space(4))) uint32_t*)(uintptr_t)src_entry;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(VarEntry) / 4); ++i) words[i] = src[i];
  __builtin_memcpy(&e, words, sizeof(VarEntry));
#else
  e = *src_entry;
#endif
}
// Packed slides: the slide is the last entry whose item_begin <= item (every slide has items: L_i >= 1), then
// (segment, head, tile) within it.  item derives from blockIdx alone, so the search and the entry are wave-uniform.
template <int D>
GP_DEV int make_view(const VarArgs& a, int64_t item, View& w) {
  const int it = (int)item;
  int lo = 0, hi = a.nslide - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (it >= a.tab[mid].item_begin) lo = mid; else hi = mid - 1;
  }
  lo = __builtin_amdgcn_readfirstlane(lo);
  VarEntry e;
  load_entry_scalar(a.tab + lo, e);
  const int local = it - e.item_begin;
  const int tile = local % e.ntile;
  const int nh = local / e.ntile;
  const int n = nh / a.H, h = nh % a.H;
  dil_view<D>(a, e.g, e.L, e.tok0, e.o_off, e.lse_off, n, h, w);
  return tile;
}

GP_DEV void add_f32x4(float* p, f32x4 v, float c) {                      // read-add-write, 16-byte aligned
  f32x4* q = reinterpret_cast<f32x4*>(p);
  *q = *q + v * c;
}

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
  // tile 0: rows of x0 (stride rs0, n0 valid rows), tile 1: rows of x1 (rs1, n1)
  GP_DEV void load(const uint16_t* x0, int64_t rs0, int n0, const uint16_t* x1, int64_t rs1, int n1, int row0) {
#pragma unroll
    for (int u = 0; u < LPT; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int tsel = idx / (kTile * CH);
      const int rem = idx % (kTile * CH);
      const int row = rem / CH, ch = rem % CH;
      uint4 z = make_uint4(0, 0, 0, 0);
      if (row0 + row < (tsel ? n1 : n0))
        z = *reinterpret_cast<const uint4*>((tsel ? x1 : x0) + (int64_t)(row0 + row) * (tsel ? rs1 : rs0) + ch * 8);
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
template <int D, bool kH, class Args>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const Args a) {
  constexpr bool kDil = !std::is_same_v<Args, BwdArgs>;     // the dilated addressings: DilArgs, VarArgs
  using TS = TileStage<D>;
  constexpr int DT = D / 16, ROWB = TS::ROWB, TILEB = TS::TILEB;
  __shared__ __attribute__((aligned(16))) char smem[4 * TILEB];   // [K0 | V0 | K1 | V1]

  const int64_t item = xcd_group(blockIdx.x, gridDim.x);
  View vw;
  const int tile = make_view<D>(a, item, vw);
  const int L = vw.nk;                               // keys; the seam's seqlen
  const int nst = vw.nk < vw.nq ? vw.nk : vw.nq;     // rows whose dq is stored
  if constexpr (kDil)
    if (tile * kOwn >= vw.nq || L == 0) return;      // no row with a dout here (delta is written for all of them)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int64_t rs = vw.rs;
  const uint16_t* kb = vw.k;
  const uint16_t* vb = vw.v;
  const int q0 = tile * kOwn + w * (kSub * 16);

  // Q / dO fragments (B operands: column = query l16), delta and lse of the wave's rows
  RowFrag<D> qf[kSub], dof[kSub];
  float lse2[kSub], dl[kSub];
#pragma unroll
  for (int qt = 0; qt < kSub; ++qt) {
    const int i = q0 + qt * 16 + l16;
    const bool valid = i < vw.nq;                    // carries a dout (a zero-pad query past nk: q = 0)
    load_rowfrag<D>(qf[qt], reinterpret_cast<const char*>(vw.q + (int64_t)i * rs), g4, i < vw.nk);
    load_rowfrag<D>(dof[qt], reinterpret_cast<const char*>(vw.dout + (int64_t)i * vw.rso), g4, valid);
    RowFrag<D> of;
    load_rowfrag<D>(of, reinterpret_cast<const char*>(vw.o + (int64_t)i * vw.rso), g4, valid);
    // delta: the diagonal of O.dO^T, summed exactly as dP sums dO.V^T
    const f32x4 dd = dot_rows<D, kH>(of, dof[qt], f32x4{0.f, 0.f, 0.f, 0.f});
    const int r = l16 & 3;
    const float pick = r == 0 ? dd[0] : r == 1 ? dd[1] : r == 2 ? dd[2] : dd[3];   // lane g4 == l16 / 4 holds it
    dl[qt] = __shfl(pick, ((l16 >> 2) << 4) | l16, 64);
    if constexpr (!kDil)
      if (valid && g4 == 0) vw.delta[i] = dl[qt];
    lse2[qt] = valid ? vw.lse[i] * kLog2e : INFINITY;
  }

  f32x4 acc[kSub][DT];
#pragma unroll
  for (int qt = 0; qt < kSub; ++qt)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // kDil: delta from the forward's o carries that kernel's own error (P rounded before P.V, o rounded), and an error
  // of delta is the same for every key of the row, so it does not average out in dq.  With the recomputed fp32 P,
  // delta* = sum_j P_ij dP_ij over all keys (zero pads: dP = 0), so eps_i = sum_j P_ij (dP_ij - delta_i) is the error
  // of delta_i, at no extra product: the lane sums its fp32 dS below.  dq is then corrected to first order by
  // -eps_i sum_j P_ij k_j (pk, one more accumulator set) and delta_i + eps_i is what the dK/dV kernel gets.  One key
  // (L = 1): dS = 0 exactly, so eps = 0 and nothing changes.  dS also enters its product as a pair of 16-bit values
  // (the rounded dS and the rounded remainder), so that dq carries the one rounding of the store and little else:
  // an error of dq at the largest elements is otherwise a rounding of the sum plus the operand roundings, which
  // per-branch results (smaller numbers, finer ulps) do not show.
  f32x4 pk[kDil ? kSub : 1][kDil ? DT : 1];
  float eps[kSub];
#pragma unroll
  for (int qt = 0; qt < kSub; ++qt) eps[qt] = 0.f;
  if constexpr (kDil) {
#pragma unroll
    for (int qt = 0; qt < kSub; ++qt)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) pk[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  TS st;
  const int ntiles = (L + kTile - 1) / kTile;
  st.load(kb, rs, L, vb, rs, L, 0);
  st.store(smem);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int kv0 = t * kTile;
    if (t + 1 < ntiles) st.load(kb, rs, L, vb, rs, L, kv0 + kTile);
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
      bf16x8 dsf[kSub], pf[kDil ? kSub : 1], dsl[kDil ? kSub : 1];
#pragma unroll
      for (int qt = 0; qt < kSub; ++qt)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float p = __builtin_amdgcn_exp2f(fmaf(sacc[qt][kt][r], a.c_log2, -lse2[qt]));
            if (tail) p = (kv0 + 32 * u + 16 * kt + 4 * g4 + r < L) ? p : 0.f;
            const float ds = p * (dpacc[qt][kt][r] - dl[qt]);
            const uint16_t dsb = f2e<kH>(ds);
            dsf[qt][4 * kt + r] = __builtin_bit_cast(__bf16, dsb);
            if constexpr (kDil) {
              eps[qt] += ds;
              pf[qt][4 * kt + r] = f2e_slot<kH>(p);
              dsl[qt][4 * kt + r] = f2e_slot<kH>(ds - e2f<kH>(dsb));   // what the rounding of dS dropped
            }
          }
      // dQ^T[d][q] += K^T[d][key] . dS^T[key][q]   (kDil: and pk^T[d][q] += K^T[d][key] . P^T[key][q])
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 kT = read_transposed<ROWB>(Kb, 32 * u, dt, l16, g4);
#pragma unroll
        for (int qt = 0; qt < kSub; ++qt) {
          acc[qt][dt] = mfma32<kH>(kT, dsf[qt], acc[qt][dt]);
          if constexpr (kDil) {
            acc[qt][dt] = mfma32<kH>(kT, dsl[qt], acc[qt][dt]);
            pk[qt][dt] = mfma32<kH>(kT, pf[qt], pk[qt][dt]);
          }
        }
      }
    }
    if (t + 1 < ntiles) st.store(smem + (2 * ((t + 1) & 1)) * TILEB);
    __syncthreads();
  }

  if constexpr (kDil) {
#pragma unroll
    for (int qt = 0; qt < kSub; ++qt) {
      // the lanes g4 = 0..3 of a query hold its keys 4 g4 + reg of every sub-tile; the zero pads add P (0 - delta)
      float e = eps[qt];
      e += __shfl_xor(e, 16, 64);
      e += __shfl_xor(e, 32, 64);
      e -= (float)vw.npad * __builtin_amdgcn_exp2f(-lse2[qt]) * dl[qt];
      const int i = q0 + qt * 16 + l16;
      if (i < vw.nq && g4 == 0) vw.delta[i] = dl[qt] + e;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[qt][dt] = acc[qt][dt] - pk[qt][dt] * e;
    }
  }

#pragma unroll
  for (int qt = 0; qt < kSub; ++qt) {
    const int i = q0 + qt * 16 + l16;
    if (i < nst) {
      if constexpr (kDil) {
        float* row = vw.gq + (int64_t)i * vw.grs;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) add_f32x4(row + 16 * dt + 4 * g4, acc[qt][dt], a.c);
      } else {
        uint16_t* row = vw.dq + (int64_t)i * rs;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const float vv[4] = {acc[qt][dt][0] * a.c, acc[qt][dt][1] * a.c, acc[qt][dt][2] * a.c, acc[qt][dt][3] * a.c};
          store_e<kH, 4>(row + 16 * dt + 4 * g4, vv);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// dK / dV: one workgroup per 128 keys of a (batch, head).
template <int D, bool kH, class Args>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const Args a) {
  constexpr bool kDil = !std::is_same_v<Args, BwdArgs>;     // the dilated addressings: DilArgs, VarArgs
  using TS = TileStage<D>;
  constexpr int DT = D / 16, ROWB = TS::ROWB, TILEB = TS::TILEB;
  constexpr int STATB = 2 * kTile * 4;                            // lse * log2(e) | delta of a query tile
  __shared__ __attribute__((aligned(16))) char smem[4 * TILEB + 2 * STATB];   // [Q0 | dO0 | Q1 | dO1 | stat0 | stat1]

  const int64_t item = xcd_group(blockIdx.x, gridDim.x);
  View vw;
  const int tile = make_view<D>(a, item, vw);
  const int L = vw.nq;                               // query rows that carry a dout; the seam's seqlen
  const int nkey = vw.nk;
  if constexpr (kDil)
    if (tile * kOwn >= nkey || L == 0) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int64_t rs = vw.rs;
  const uint16_t* qb = vw.q;
  const uint16_t* dob = vw.dout;
  const float* lseb = vw.lse;
  const float* delb = vw.delta;
  const int k0 = tile * kOwn + w * (kSub * 16);

  // K / V fragments (B operands: column = key l16) of the wave's keys
  RowFrag<D> kf[kSub], vf[kSub];
#pragma unroll
  for (int kt = 0; kt < kSub; ++kt) {
    const int key = k0 + kt * 16 + l16;
    load_rowfrag<D>(kf[kt], reinterpret_cast<const char*>(vw.k + (int64_t)key * rs), g4, key < nkey);
    load_rowfrag<D>(vf[kt], reinterpret_cast<const char*>(vw.v + (int64_t)key * rs), g4, key < nkey);
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
  st.load(qb, rs, nkey, dob, vw.rso, L, 0);          // a query row past nkey is a zero pad
  load_stat(0);
  st.store(smem);
  store_stat(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) {
      st.load(qb, rs, nkey, dob, vw.rso, L, (t + 1) * kTile);
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
    if (key < nkey) {
      if constexpr (kDil) {
        const int64_t off = (int64_t)key * vw.grs;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          add_f32x4(vw.gk + off + 16 * dt + 4 * g4, dkacc[kt][dt], a.c);
          add_f32x4(vw.gv + off + 16 * dt + 4 * g4, dvacc[kt][dt], 1.f);
        }
      } else {
        const int64_t off = (int64_t)key * rs;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const float kk[4] = {dkacc[kt][dt][0] * a.c, dkacc[kt][dt][1] * a.c, dkacc[kt][dt][2] * a.c, dkacc[kt][dt][3] * a.c};
          const float vv[4] = {dvacc[kt][dt][0], dvacc[kt][dt][1], dvacc[kt][dt][2], dvacc[kt][dt][3]};
          store_e<kH, 4>(vw.dk + off + 16 * dt + 4 * g4, kk);
          store_e<kH, 4>(vw.dv + off + 16 * dt + 4 * g4, vv);
        }
      }
    }
  }
}

template <int D, bool kH>
void launch_bwd(const BwdArgs& a, unsigned grid, hipStream_t s) {
  attn_bwd_dq_kernel<D, kH, BwdArgs><<<grid, 256, 0, s>>>(a);
  attn_bwd_dkv_kernel<D, kH, BwdArgs><<<grid, 256, 0, s>>>(a);
}

bool bwd_dim_ok(int D) { return D == 48 || D == 64 || D == 96; }

// ---------------------------------------------------------------------------------------
// Backward of the merge without its LayerNorm (DilatedAttention.scattering, dilated_attention.py:100-131), one
// thread per (token, head): the branch weights are gp_branch_merge_ln's (uncovered or lse == 0 -> -1e8, fp32
// softmax over the branches by v_exp_f32 / v_rcp_f32) and take no gradient (:119-124, torch.no_grad()), so the
// sparse row (n, i, h) whose merge slot is the token receives dout_b = w_b dmerged, rounded to the format as the
// MFMA operand it is.  Covered (token, head)s and sparse rows with a slot below L correspond one to one: every
// dout row the attention kernels read is written here, and no row the forward left unwritten is read.
struct MergeBwdArgs {
  const float* lse[GP_MAX_BRANCHES];
  uint16_t* dout[GP_MAX_BRANCHES];
  GpBranch g[GP_MAX_BRANCHES];
  const uint16_t* dmerged;
  int64_t B, L;
  int32_t H, nbranch;
};

// Token p, head h of one sequence (a batch element, or a packed slide).  region(b, g, lse, dout) gives branch b's
// geometry for that sequence and the bases of the sequence's regions in the branch's lse and dout buffers; dm is the
// (token, head)'s D elements of dmerged.
template <int D, bool kH, class F>
GP_DEV void merge_bwd_token(int nbranch, int H, int p, int h, const uint16_t* dm, F region) {
  float e[GP_MAX_BRANCHES];
  uint16_t* drows[GP_MAX_BRANCHES];                      // the dout row (D elements)
  bool cov[GP_MAX_BRANCHES];
  float mx = -INFINITY;
#pragma unroll
  for (int b = 0; b < GP_MAX_BRANCHES; ++b) {
    e[b] = -1e8f; cov[b] = false; drows[b] = nullptr;
    if (b < nbranch) {
      GpBranch g;
      const float* lse;
      uint16_t* dout;
      region(b, g, lse, dout);
      const int n = p / g.g, pt = p - n * g.g;
      const int i = pt / g.r, j = pt - i * g.r;
      cov[b] = h / g.hpg == j;
      drows[b] = dout + (((int64_t)n * g.m + i) * H + h) * D;
      if (cov[b]) e[b] = lse[((int64_t)n * H + h) * g.m + i];
      if (!cov[b] || e[b] == 0.f) e[b] = -1e8f;            // dilated_attention.py:46
      mx = fmaxf(mx, e[b]);
    }
  }
  float wsum = 0.f;
#pragma unroll
  for (int b = 0; b < GP_MAX_BRANCHES; ++b)
    if (b < nbranch) {
      e[b] = __builtin_amdgcn_exp2f((e[b] - mx) * kLog2e);
      wsum += e[b];
    }
  const float inv = __builtin_amdgcn_rcpf(wsum);
#pragma unroll
  for (int b = 0; b < GP_MAX_BRANCHES; ++b)
    if (b < nbranch && cov[b]) {
      const float wb = e[b] * inv;
      uint16_t* drow = drows[b];
#pragma unroll
      for (int c = 0; c < D; c += 8) {
        float x[8];
        load_e<kH, 8>(dm + c, x);
        *reinterpret_cast<uint4*>(drow + c) = make_uint4(pack2e<kH>(x[0] * wb, x[1] * wb), pack2e<kH>(x[2] * wb, x[3] * wb),
                                                         pack2e<kH>(x[4] * wb, x[5] * wb), pack2e<kH>(x[6] * wb, x[7] * wb));
      }
    }
}

template <int D, bool kH>
__global__ __launch_bounds__(256) void merge_bwd_kernel(const MergeBwdArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.B * a.L * a.H) return;
  const int h = (int)(idx % a.H);
  const int64_t tok = idx / a.H;
  const int bidx = (int)(tok / a.L), p = (int)(tok % a.L);
  merge_bwd_token<D, kH>(a.nbranch, a.H, p, h, a.dmerged + (tok * a.H + h) * D,
                         [&](int b, GpBranch& g, const float*& lse, uint16_t*& dout) {
                           g = a.g[b];
                           const int64_t seg0 = (int64_t)bidx * g.nseg;
                           lse = a.lse[b] + seg0 * a.H * g.m;
                           dout = a.dout[b] + seg0 * g.m * a.H * D;
                         });
}

// The merge backward of packed slides: one thread per (packed token, head); the slide is the last one whose first
// row tok0 <= token (branch 0's entries), the geometry and the region bases come from the (branch, slide) entries.
struct VarMergeArgs {
  const float* lse[GP_MAX_BRANCHES];
  uint16_t* dout[GP_MAX_BRANCHES];
  const VarEntry* tab;           // [nbranch][nslide]
  const uint16_t* dmerged;       // [T, H*D]
  int64_t T;
  int32_t nslide, H, nbranch;
};

template <int D, bool kH>
__global__ __launch_bounds__(256) void merge_bwd_varlen_kernel(const VarMergeArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.T * a.H) return;
  const int h = (int)(idx % a.H);
  const int64_t tok = idx / a.H;
  int lo = 0, hi = a.nslide - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tok >= a.tab[mid].tok0) lo = mid; else hi = mid - 1;
  }
  const int p = (int)(tok - a.tab[lo].tok0);
  merge_bwd_token<D, kH>(a.nbranch, a.H, p, h, a.dmerged + (tok * a.H + h) * D,
                         [&](int b, GpBranch& g, const float*& lse, uint16_t*& dout) {
                           const VarEntry& e = a.tab[(int64_t)b * a.nslide + lo];
                           g = e.g;
                           lse = a.lse[b] + e.lse_off;
                           dout = a.dout[b] + e.o_off;
                         });
}

// The one rounding of the accumulated gradients: g [rows, 3, E] fp32 planes -> dq / dk / dv rows (stride ds).
template <bool kH>
__global__ __launch_bounds__(256) void grad_store_kernel(const float* gq, const float* gk, const float* gv,
                                                         uint16_t* dq, uint16_t* dk, uint16_t* dv, int64_t ds,
                                                         int64_t rows, int E) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int cpr = E / 4;
  if (idx >= rows * cpr) return;
  const int64_t r = idx / cpr;
  const int c = (int)(idx % cpr) * 4;
  float v[4];
  load_f32<4>(gq + r * E + c, v);
  store_e<kH, 4>(dq + r * ds + c, v);
  load_f32<4>(gk + r * E + c, v);
  store_e<kH, 4>(dk + r * ds + c, v);
  load_f32<4>(gv + r * E + c, v);
  store_e<kH, 4>(dv + r * ds + c, v);
}

// gp_dilated_attn_bwd's workspace: per branch dout_b (16-bit) and delta_b (fp32), then the three fp32 accumulators
struct DilWs {
  size_t dout[GP_MAX_BRANCHES], delta[GP_MAX_BRANCHES], g[3], total;
  GpBranch geo[GP_MAX_BRANCHES];
};
bool dil_ws_layout(int64_t B, int64_t L, int H, int D, const int32_t* seg_len, const int32_t* ratios, int nbranch,
                   DilWs& w) {
  if (B <= 0 || L <= 0 || H <= 0 || H > 4096 || !bwd_dim_ok(D) || !seg_len || !ratios || nbranch < 1 ||
      nbranch > GP_MAX_BRANCHES)
    return false;
  if (B > (int64_t)0x7fffffff / L) return false;            // B * L below 2^31
  uint64_t off = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t at = off;
    off += (bytes + 255) / 256 * 256;
    return (size_t)at;
  };
  for (int b = 0; b < nbranch; ++b) {
    if (seg_len[b] <= 0 || ratios[b] <= 0) return false;
    w.geo[b] = gp_make_branch(L, seg_len[b], ratios[b], H);
    const uint64_t rows = (uint64_t)B * w.geo[b].nseg * w.geo[b].m * H;
    w.dout[b] = take(rows * D * sizeof(uint16_t));
    w.delta[b] = take(rows * sizeof(float));
  }
  for (int i = 0; i < 3; ++i) w.g[i] = take((uint64_t)B * L * H * D * sizeof(float));
  w.total = (size_t)off;
  return true;
}

template <int D, bool kH>
void launch_dil_bwd(const MergeBwdArgs& m, DilArgs a, const DilWs& w, char* ws, const uint16_t* const* o_in, int64_t B, uint16_t* dq,
                    uint16_t* dk, uint16_t* dv, int64_t ds, hipStream_t s) {
  const int64_t th = B * m.L * m.H;
  merge_bwd_kernel<D, kH><<<(unsigned)((th + 255) / 256), 256, 0, s>>>(m);
  for (int b = 0; b < m.nbranch; ++b) {                    // fixed order: each branch adds into the accumulators
    a.g = w.geo[b];
    a.o = o_in[b];
    a.dout = m.dout[b];
    a.lse = m.lse[b];
    a.delta = reinterpret_cast<float*>(ws + w.delta[b]);
    a.ntile = (a.g.m + kOwn - 1) / kOwn;
    const unsigned grid = (unsigned)(B * a.g.nseg * m.H * a.ntile);
    attn_bwd_dq_kernel<D, kH, DilArgs><<<grid, 256, 0, s>>>(a);
    attn_bwd_dkv_kernel<D, kH, DilArgs><<<grid, 256, 0, s>>>(a);
  }
  const int E = m.H * D;
  const int64_t n4 = B * m.L * (E / 4);
  grad_store_kernel<kH><<<(unsigned)((n4 + 255) / 256), 256, 0, s>>>(a.gq, a.gk, a.gv, dq, dk, dv, ds, B * m.L, E);
}

// gp_varlen_bwd_plan's buffer: this header (host side only), then the [nbranch][nslide] VarEntry table the kernels
// read from the device copy.  Its first fields, up to items, are public (include/gigapath_hip.h).
constexpr int32_t kVarBwdMagic = 0x47504231;   // "GPB1"
struct VarBwdHdr {
  int32_t magic, nslide, nbranch, H, D, reserved;
  int64_t T;
  int64_t items[GP_MAX_BRANCHES];              // work items of each branch's two attention launches
  int64_t qkv_stride;
  const uint16_t* qkv;
  const uint16_t* o[GP_MAX_BRANCHES];
  const float* lse[GP_MAX_BRANCHES];
  int64_t ws_dout[GP_MAX_BRANCHES], ws_delta[GP_MAX_BRANCHES], ws_g[3], ws_total;
  int64_t tab_off, bytes;
};
inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
void var_bwd_layout(int nslide, int nbranch, VarBwdHdr& h) {
  h.tab_off = align_up((int64_t)sizeof(VarBwdHdr), 16);
  h.bytes = align_up(h.tab_off + (int64_t)nslide * nbranch * (int64_t)sizeof(VarEntry), 16);
}

template <int D, bool kH>
void launch_var_bwd(const VarBwdHdr& h, const VarEntry* tab, char* ws, const uint16_t* dmerged, float c, float c_log2,
                    uint16_t* dq, uint16_t* dk, uint16_t* dv, int64_t ds, hipStream_t s) {
  const int E = h.H * D;
  VarMergeArgs m = {};
  for (int b = 0; b < h.nbranch; ++b) {
    m.lse[b] = h.lse[b];
    m.dout[b] = reinterpret_cast<uint16_t*>(ws + h.ws_dout[b]);
  }
  m.tab = tab; m.dmerged = dmerged; m.T = h.T;
  m.nslide = h.nslide; m.H = h.H; m.nbranch = h.nbranch;
  merge_bwd_varlen_kernel<D, kH><<<(unsigned)((h.T * h.H + 255) / 256), 256, 0, s>>>(m);
  VarArgs a = {};
  a.q = h.qkv; a.k = h.qkv + E; a.v = h.qkv + 2 * E;
  a.gq = reinterpret_cast<float*>(ws + h.ws_g[0]);
  a.gk = reinterpret_cast<float*>(ws + h.ws_g[1]);
  a.gv = reinterpret_cast<float*>(ws + h.ws_g[2]);
  a.row_stride = h.qkv_stride; a.nslide = h.nslide; a.H = h.H;
  a.c = c; a.c_log2 = c_log2;
  for (int b = 0; b < h.nbranch; ++b) {                    // fixed order: each branch adds into the accumulators
    a.o = h.o[b];
    a.dout = m.dout[b];
    a.lse = h.lse[b];
    a.delta = reinterpret_cast<float*>(ws + h.ws_delta[b]);
    a.tab = tab + (int64_t)b * h.nslide;
    const unsigned grid = (unsigned)h.items[b];
    attn_bwd_dq_kernel<D, kH, VarArgs><<<grid, 256, 0, s>>>(a);
    attn_bwd_dkv_kernel<D, kH, VarArgs><<<grid, 256, 0, s>>>(a);
  }
  const int64_t n4 = h.T * (E / 4);
  grad_store_kernel<kH><<<(unsigned)((n4 + 255) / 256), 256, 0, s>>>(a.gq, a.gk, a.gv, dq, dk, dv, ds, h.T, E);
}

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

extern "C" size_t gp_dilated_attn_bwd_workspace_bytes(int64_t B, int64_t L, int H, int D, const int32_t* seg_len,
                                                      const int32_t* ratios, int nbranch) {
  DilWs w;
  return dil_ws_layout(B, L, H, D, seg_len, ratios, nbranch, w) ? w.total : 0;
}

extern "C" int gp_dilated_attn_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t row_stride,
                                   int64_t B, int64_t L, int H, int D, const int32_t* seg_len, const int32_t* ratios,
                                   int nbranch, const uint16_t* const* o_in, const float* const* lse_in,
                                   const uint16_t* dmerged, float softmax_scale, int q_log2_prescaled, uint16_t* dq,
                                   uint16_t* dk, uint16_t* dv, int64_t d_row_stride, void* workspace,
                                   size_t workspace_bytes, int fmt, void* stream) {
  GP_REQUIRE(bwd_dim_ok(D), "gp_dilated_attn_bwd: head dim %d unsupported (D in {48, 64, 96})", D);
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16, "gp_dilated_attn_bwd: bad fmt %d (GP_FMT_BF16 or GP_FMT_F16)", fmt);
  GP_REQUIRE(!q_log2_prescaled || D != 96, "gp_dilated_attn_bwd: q_log2_prescaled needs D in {48, 64} (D = %d)", D);
  GP_REQUIRE(nbranch >= 1 && nbranch <= GP_MAX_BRANCHES, "gp_dilated_attn_bwd: nbranch must be 1..%d (got %d)",
             GP_MAX_BRANCHES, nbranch);
  GP_REQUIRE(B > 0 && L > 0 && H > 0 && H <= 4096 && B <= (int64_t)0x7fffffff / L,
             "gp_dilated_attn_bwd: bad sizes B %lld, L %lld, H %d", (long long)B, (long long)L, H);
  const void* ptrs[] = {q, k, v, dmerged, dq, dk, dv};
  const char* names[] = {"q", "k", "v", "dmerged", "dq", "dk", "dv"};
  for (int i = 0; i < 7; ++i) {
    GP_REQUIRE(ptrs[i] != nullptr, "gp_dilated_attn_bwd: null pointer (%s)", names[i]);
    GP_REQUIRE(gp_aligned(ptrs[i], 16), "gp_dilated_attn_bwd: misaligned pointer (%s)", names[i]);
  }
  GP_REQUIRE(seg_len && ratios && o_in && lse_in, "gp_dilated_attn_bwd: null pointer (%s)",
             !seg_len ? "seg_len" : !ratios ? "ratios" : !o_in ? "o_in" : "lse_in");
  const int64_t E = (int64_t)H * D;
  GP_REQUIRE(row_stride >= E && row_stride % 8 == 0, "gp_dilated_attn_bwd: row_stride %lld below H*D = %lld or not a multiple of 8",
             (long long)row_stride, (long long)E);
  GP_REQUIRE(d_row_stride >= E && d_row_stride % 8 == 0,
             "gp_dilated_attn_bwd: d_row_stride %lld below H*D = %lld or not a multiple of 8", (long long)d_row_stride,
             (long long)E);
  for (int b = 0; b < nbranch; ++b) {
    GP_REQUIRE(seg_len[b] > 0 && ratios[b] > 0, "gp_dilated_attn_bwd: branch %d: bad seg_len %d / ratio %d", b,
               seg_len[b], ratios[b]);
    GP_REQUIRE(o_in[b] != nullptr && lse_in[b] != nullptr, "gp_dilated_attn_bwd: null pointer (o_in / lse_in [%d])", b);
    GP_REQUIRE(gp_aligned(o_in[b], 16) && gp_aligned(lse_in[b], 4),
               "gp_dilated_attn_bwd: misaligned pointer (o_in / lse_in [%d])", b);
  }
  DilWs w;
  GP_REQUIRE(dil_ws_layout(B, L, H, D, seg_len, ratios, nbranch, w), "gp_dilated_attn_bwd: bad shape");
  GP_REQUIRE(workspace != nullptr && workspace_bytes >= w.total,
             "gp_dilated_attn_bwd: workspace too small (%zu bytes, gp_dilated_attn_bwd_workspace_bytes asks %zu)",
             workspace ? workspace_bytes : (size_t)0, w.total);
  GP_REQUIRE(gp_aligned(workspace, 16), "gp_dilated_attn_bwd: misaligned workspace (16 bytes)");
  for (int b = 0; b < nbranch; ++b) {
    const int64_t items = B * w.geo[b].nseg * H * ((w.geo[b].m + kOwn - 1) / kOwn);
    GP_REQUIRE(items < (int64_t)0x7fffffff, "gp_dilated_attn_bwd: branch %d: %lld work items exceed one launch", b,
               (long long)items);
  }
  GP_REQUIRE((B * L * H + 255) / 256 < (int64_t)0x7fffffff && (B * L * (E / 4) + 255) / 256 < (int64_t)0x7fffffff,
             "gp_dilated_attn_bwd: B*L*H*D too large for one launch");

  char* ws = static_cast<char*>(workspace);
  MergeBwdArgs m = {};
  for (int b = 0; b < nbranch; ++b) {
    m.lse[b] = lse_in[b];
    m.dout[b] = reinterpret_cast<uint16_t*>(ws + w.dout[b]);
    m.g[b] = w.geo[b];
  }
  m.dmerged = dmerged;
  m.B = B; m.L = L; m.H = H; m.nbranch = nbranch;
  DilArgs a = {};
  a.q = q; a.k = k; a.v = v;
  a.gq = reinterpret_cast<float*>(ws + w.g[0]);
  a.gk = reinterpret_cast<float*>(ws + w.g[1]);
  a.gv = reinterpret_cast<float*>(ws + w.g[2]);
  a.row_stride = row_stride; a.L = L; a.H = H;
  if (q_log2_prescaled) {            // logits are q'.k in the log2 domain: dq' = ln 2 dS k, dk = ln 2 dS^T q'
    a.c = 0.6931471805599453f;
    a.c_log2 = 1.f;
  } else {
    a.c = softmax_scale > 0.f ? softmax_scale : 1.0f / sqrtf((float)D);
    a.c_log2 = a.c * kLog2e;
  }
  hipStream_t s = gp_stream(stream);
  // the accumulators start at zero: a (token, head) no branch covers keeps it
  const hipError_t me = hipMemsetAsync(ws + w.g[0], 0, w.total - w.g[0], s);
  if (me != hipSuccess) {
    gp_set_error("gp_dilated_attn_bwd: hipMemsetAsync: %s", hipGetErrorString(me));
    return (int)me;
  }
  const bool kh = fmt == GP_FMT_F16;
  switch (D) {
    case 48: if (kh) launch_dil_bwd<48, true>(m, a, w, ws, o_in, B, dq, dk, dv, d_row_stride, s); else launch_dil_bwd<48, false>(m, a, w, ws, o_in, B, dq, dk, dv, d_row_stride, s); break;
    case 64: if (kh) launch_dil_bwd<64, true>(m, a, w, ws, o_in, B, dq, dk, dv, d_row_stride, s); else launch_dil_bwd<64, false>(m, a, w, ws, o_in, B, dq, dk, dv, d_row_stride, s); break;
    default: if (kh) launch_dil_bwd<96, true>(m, a, w, ws, o_in, B, dq, dk, dv, d_row_stride, s); else launch_dil_bwd<96, false>(m, a, w, ws, o_in, B, dq, dk, dv, d_row_stride, s); break;
  }
  return gp_check_launch("gp_dilated_attn_bwd");
}

// ---------------------------------------------------------------------------------------
// Packed slides (varlen): the plan holds the host header and the device table; the launch call copies nothing.
extern "C" int64_t gp_varlen_bwd_plan_bytes(int nslide, int nbranch) {
  if (nslide < 1 || nbranch < 1 || nbranch > GP_MAX_BRANCHES) return -1;
  VarBwdHdr h;
  var_bwd_layout(nslide, nbranch, h);
  return h.bytes;
}

extern "C" int gp_varlen_bwd_plan(const int64_t* L, int nslide, int H, int D, const int32_t* seg_len,
                                  const int32_t* ratios, int nbranch, const uint16_t* qkv, int64_t qkv_row_stride,
                                  const uint16_t* const* o_in, const float* const* lse_in, void* plan_host,
                                  int64_t plan_bytes, int64_t* workspace_bytes) {
  GP_REQUIRE(L && seg_len && ratios && workspace_bytes, "gp_varlen_bwd_plan: null pointer (%s)",
             !L ? "L" : !seg_len ? "seg_len" : !ratios ? "ratios" : "workspace_bytes");
  GP_REQUIRE(nslide >= 1, "gp_varlen_bwd_plan: nslide must be >= 1 (got %d)", nslide);
  GP_REQUIRE(nbranch >= 1 && nbranch <= GP_MAX_BRANCHES, "gp_varlen_bwd_plan: nbranch must be 1..%d (got %d)",
             GP_MAX_BRANCHES, nbranch);
  GP_REQUIRE(D == 48, "gp_varlen_bwd_plan: head dim %d unsupported (the varlen kernels cover D = 48)", D);
  GP_REQUIRE(H > 0 && H <= 4096, "gp_varlen_bwd_plan: bad H %d", H);
  const int64_t E = (int64_t)H * D;
  GP_REQUIRE(qkv_row_stride >= 3 * E && qkv_row_stride % 8 == 0,
             "gp_varlen_bwd_plan: qkv_row_stride %lld below 3*H*D = %lld or not a multiple of 8",
             (long long)qkv_row_stride, (long long)(3 * E));
  int64_t T = 0;
  for (int i = 0; i < nslide; ++i) {
    GP_REQUIRE(L[i] > 0 && L[i] < (int64_t)0x7fffffff, "gp_varlen_bwd_plan: slide %d has L = %lld", i, (long long)L[i]);
    T += L[i];
    GP_REQUIRE(T < (int64_t)0x7fffffff, "gp_varlen_bwd_plan: %lld packed tokens exceed 2^31 - 1", (long long)T);
  }
  GP_REQUIRE((T * H + 255) / 256 < (int64_t)0x7fffffff && (T * (E / 4) + 255) / 256 < (int64_t)0x7fffffff,
             "gp_varlen_bwd_plan: T*H*D too large for one launch");
  VarBwdHdr h;
  memset(&h, 0, sizeof(h));
  var_bwd_layout(nslide, nbranch, h);
  uint64_t off = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t at = off;
    off += (bytes + 255) / 256 * 256;
    return (int64_t)at;
  };
  for (int b = 0; b < nbranch; ++b) {
    GP_REQUIRE(seg_len[b] > 0 && ratios[b] > 0, "gp_varlen_bwd_plan: branch %d: bad seg_len %d / ratio %d", b, seg_len[b],
               ratios[b]);
    uint64_t rows = 0;                                      // (sparse row, head)s of every slide
    int64_t items = 0;
    for (int i = 0; i < nslide; ++i) {
      const GpBranch g = gp_make_branch(L[i], seg_len[b], ratios[b], H);
      rows += (uint64_t)g.nseg * g.m * H;
      items += (int64_t)g.nseg * H * ((g.m + kOwn - 1) / kOwn);
      GP_REQUIRE(items < (int64_t)0x7fffffff, "gp_varlen_bwd_plan: branch %d: %lld work items exceed one launch", b,
                 (long long)items);
    }
    h.items[b] = items;
    h.ws_dout[b] = take(rows * D * sizeof(uint16_t));
    h.ws_delta[b] = take(rows * sizeof(float));
  }
  for (int i = 0; i < 3; ++i) h.ws_g[i] = take((uint64_t)T * E * sizeof(float));
  h.ws_total = (int64_t)off;
  *workspace_bytes = h.ws_total;
  if (plan_host == nullptr) return 0;                       // sizing call

  GP_REQUIRE(plan_bytes >= h.bytes, "gp_varlen_bwd_plan: plan buffer %lld < %lld bytes (gp_varlen_bwd_plan_bytes)",
             (long long)plan_bytes, (long long)h.bytes);
  GP_REQUIRE(gp_aligned(plan_host, 8), "gp_varlen_bwd_plan: misaligned pointer (plan_host, 8 bytes)");
  GP_REQUIRE(qkv != nullptr && o_in != nullptr && lse_in != nullptr, "gp_varlen_bwd_plan: null pointer (%s)",
             !qkv ? "qkv" : !o_in ? "o_in" : "lse_in");
  GP_REQUIRE(gp_aligned(qkv, 16), "gp_varlen_bwd_plan: misaligned pointer (qkv)");
  for (int b = 0; b < nbranch; ++b) {
    GP_REQUIRE(o_in[b] != nullptr && lse_in[b] != nullptr, "gp_varlen_bwd_plan: null pointer (o_in / lse_in [%d])", b);
    GP_REQUIRE(gp_aligned(o_in[b], 16) && gp_aligned(lse_in[b], 4),
               "gp_varlen_bwd_plan: misaligned pointer (o_in / lse_in [%d])", b);
  }
  char* base = static_cast<char*>(plan_host);
  memset(base, 0, (size_t)h.bytes);
  VarEntry* tab = reinterpret_cast<VarEntry*>(base + h.tab_off);
  for (int b = 0; b < nbranch; ++b) {
    int64_t tok = 0, oo = 0, lo = 0, items = 0;
    for (int i = 0; i < nslide; ++i) {
      VarEntry& e = tab[(size_t)b * nslide + i];
      e.g = gp_make_branch(L[i], seg_len[b], ratios[b], H);
      e.ntile = (e.g.m + kOwn - 1) / kOwn;
      e.item_begin = (int32_t)items;
      e.L = L[i];
      e.tok0 = tok;
      e.o_off = oo;
      e.lse_off = lo;
      items += (int64_t)e.g.nseg * H * e.ntile;
      tok += L[i];
      oo += (int64_t)e.g.nseg * e.g.m * H * D;
      lo += (int64_t)e.g.nseg * H * e.g.m;
    }
    h.o[b] = o_in[b];
    h.lse[b] = lse_in[b];
  }
  h.magic = kVarBwdMagic;
  h.nslide = nslide; h.nbranch = nbranch; h.H = H; h.D = D;
  h.T = T;
  h.qkv_stride = qkv_row_stride;
  h.qkv = qkv;
  memcpy(base, &h, sizeof(h));
  return 0;
}

extern "C" int gp_dilated_attn_bwd_varlen(const void* plan_host, const void* plan_dev, const uint16_t* dmerged,
                                          uint16_t* dq, uint16_t* dk, uint16_t* dv, int64_t d_row_stride,
                                          void* workspace, size_t workspace_bytes, int fmt, void* stream) {
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16,
             "gp_dilated_attn_bwd_varlen: bad fmt %d (GP_FMT_BF16 or GP_FMT_F16)", fmt);
  GP_REQUIRE(plan_host != nullptr && plan_dev != nullptr, "gp_dilated_attn_bwd_varlen: null pointer (%s)",
             !plan_host ? "plan_host" : "plan_dev");
  GP_REQUIRE(gp_aligned(plan_host, 8) && gp_aligned(plan_dev, 16),
             "gp_dilated_attn_bwd_varlen: misaligned pointer (plan_host 8 bytes / plan_dev 16 bytes)");
  VarBwdHdr h;
  memcpy(&h, plan_host, sizeof(h));
  GP_REQUIRE(h.magic == kVarBwdMagic, "gp_dilated_attn_bwd_varlen: not a gp_varlen_bwd_plan buffer");
  GP_REQUIRE(h.D == 48 && h.nslide >= 1 && h.nbranch >= 1 && h.nbranch <= GP_MAX_BRANCHES && h.H > 0 && h.T > 0 &&
                 h.T < (int64_t)0x7fffffff,
             "gp_dilated_attn_bwd_varlen: corrupt plan header");
  const void* ptrs[] = {dmerged, dq, dk, dv};
  const char* names[] = {"dmerged", "dq", "dk", "dv"};
  for (int i = 0; i < 4; ++i) {
    GP_REQUIRE(ptrs[i] != nullptr, "gp_dilated_attn_bwd_varlen: null pointer (%s)", names[i]);
    GP_REQUIRE(gp_aligned(ptrs[i], 16), "gp_dilated_attn_bwd_varlen: misaligned pointer (%s)", names[i]);
  }
  const int64_t E = (int64_t)h.H * h.D;
  GP_REQUIRE(d_row_stride >= E && d_row_stride % 8 == 0,
             "gp_dilated_attn_bwd_varlen: d_row_stride %lld below H*D = %lld or not a multiple of 8",
             (long long)d_row_stride, (long long)E);
  GP_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)h.ws_total,
             "gp_dilated_attn_bwd_varlen: workspace too small (%zu bytes, gp_varlen_bwd_plan asks %zu)",
             workspace ? workspace_bytes : (size_t)0, (size_t)h.ws_total);
  GP_REQUIRE(gp_aligned(workspace, 16), "gp_dilated_attn_bwd_varlen: misaligned workspace (16 bytes)");
  for (int b = 0; b < h.nbranch; ++b)
    GP_REQUIRE(h.items[b] > 0 && h.items[b] < (int64_t)0x7fffffff,
               "gp_dilated_attn_bwd_varlen: branch %d: %lld work items exceed one launch", b, (long long)h.items[b]);

  char* ws = static_cast<char*>(workspace);
  const VarEntry* tab = reinterpret_cast<const VarEntry*>(static_cast<const char*>(plan_dev) + h.tab_off);
  hipStream_t s = gp_stream(stream);
  // the accumulators start at zero: a (token, head) no branch covers keeps it
  const hipError_t me = hipMemsetAsync(ws + h.ws_g[0], 0, (size_t)(h.ws_total - h.ws_g[0]), s);
  if (me != hipSuccess) {
    gp_set_error("gp_dilated_attn_bwd_varlen: hipMemsetAsync: %s", hipGetErrorString(me));
    return (int)me;
  }
  // the forward's q is pre-scaled (logits q'.k in the log2 domain): dq' = ln 2 dS k, dk = ln 2 dS^T q'
  const float c = 0.6931471805599453f, c_log2 = 1.f;
  if (fmt == GP_FMT_F16) launch_var_bwd<48, true>(h, tab, ws, dmerged, c, c_log2, dq, dk, dv, d_row_stride, s);
  else launch_var_bwd<48, false>(h, tab, ws, dmerged, c, c_log2, dq, dk, dv, d_row_stride, s);
  return gp_check_launch("gp_dilated_attn_bwd_varlen");
}
