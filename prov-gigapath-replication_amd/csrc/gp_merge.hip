// The LSE-weighted branch merge of dilated attention for gfx950, fused with inner_attn_ln: replaces
// DilatedAttention.scattering (torchscale/component/dilated_attention.py:100-131).  Reads the per-branch
// o / lse that the attention kernels (gp_attn.hip) write.  Three kernels: branch_merge_kernel (any registered
// width), branch_merge_v2_kernel (E = 768, D = 48, one token per wave) and branch_merge_v3_kernel (the product:
// v2's arithmetic with the LSEs staged per block).
// Every launch configuration is fixed at compile time (no run-time variant switches); measured
// alternatives live in tools/attn_lab/ (a separate build target).
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "gp_attn_plan.h"

namespace {

GP_DEV float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

struct MergeArgs {
  int64_t B, L;
  int64_t tok_lo, ntok;   // window of tokens [tok_lo, tok_lo + ntok) of every batch; out row = b*ntok + t
  int32_t H, D, E, nbranch;
  MergeBranch br[GP_MAX_BRANCHES];
  const float* ln_w;
  const float* ln_b;
  float eps;
  uint16_t* out;
  // varlen (packed slides): slide i owns packed tokens [tok_off[i], tok_off[i+1]); its branch b
  // geometry and o/lse regions are mtab[i * nbranch + b]
  const MergeBranch* mtab;
  const int64_t* tok_off;
  int32_t nslide;
  DivMagic dnt;        // division by ntok (the batch index of a row)
  // token list (branch_merge_v3_kernel kList, gp_branch_merge_ln_rows): out row b*ntok + k is token tok_list[k]
  const int32_t* tok_list;
};

// One wave per run of kTPW consecutive tokens; lane l owns the EPL = E/64 contiguous elements
// [l*EPL, (l+1)*EPL) of head l*EPL/D (EPL divides D).  The sparse_to_dense position of the
// token in every branch -- segment n, dense slot t = p mod g, sparse row i = t / r, phase
// jj = t mod r -- is wave-uniform: divided out once per run, then stepped token by token.  The
// lanes a branch covers for phase jj are the contiguous range [jj*LPH, (jj+1)*LPH), LPH = lanes
// per head group.  Math per token is that of dilated_attention.py:100-131 (fp32 weights,
// branch-order accumulation) followed by inner_attn_ln.
constexpr int kTPW = 1;

// NBR < GP_MAX_BRANCHES: the launch guarantees a.nbranch == NBR, so the branch loops have a
// compile-time trip count (the 5-branch schedule of every registered arch: 3 dead branches of
// position stepping, address math and exp fewer per token)
template <int EPL, int D, bool kTab = false, int NBR = GP_MAX_BRANCHES, bool kH = false>
__global__ __launch_bounds__(256) void branch_merge_kernel(const MergeArgs a) {
  const int nbr = NBR < GP_MAX_BRANCHES ? NBR : a.nbranch;
  const int lane = threadIdx.x & 63;
  const int run = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  const int total = (int)(a.B * a.ntok);
  const int r0 = run * kTPW;
  if (r0 >= total) return;
  // kTab: the token's slide (binary search, wave-uniform) and that slide's branch entries
  MergeBranch tb[kTab ? GP_MAX_BRANCHES : 1];
  int64_t slide_tok0 = 0;
  if constexpr (kTab) {
    int lo = 0, hi = a.nslide - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((int64_t)r0 >= a.tok_off[mid]) lo = mid; else hi = mid - 1;
    }
    slide_tok0 = a.tok_off[lo];
#pragma unroll
    for (int b = 0; b < NBR; ++b)
      if (b < nbr) tb[b] = a.mtab[lo * a.nbranch + b];
  }
  const int nt = (int)a.ntok;
  const int E = 64 * EPL;
  const int col0 = lane * EPL;
  int pn[GP_MAX_BRANCHES], pt[GP_MAX_BRANCHES], pi[GP_MAX_BRANCHES], pj[GP_MAX_BRANCHES];
  int bidx = 0, p = 0;
  for (int k = 0; k < kTPW; ++k) {
    const int row = r0 + k;
    if (row >= total) break;
    if (k == 0 || p + 1 >= (int)a.tok_lo + nt) {   // (re)derive positions: run start / next batch
      if constexpr (kTab) {
        bidx = 0;
        p = (int)(row - slide_tok0);
      } else {
        bidx = (int)div_magic((uint32_t)row, a.dnt);
        p = (int)a.tok_lo + (row - bidx * nt);
      }
#pragma unroll
      for (int b = 0; b < NBR; ++b)
        if (b < nbr) {
          const MergeBranch& mb = kTab ? tb[b] : a.br[b];
          pn[b] = (int)div_magic((uint32_t)p, mb.dg);
          pt[b] = p - pn[b] * mb.g.g;
          pi[b] = (int)div_magic((uint32_t)pt[b], mb.dr);
          pj[b] = pt[b] - pi[b] * mb.g.r;
        }
    } else {
      ++p;
#pragma unroll
      for (int b = 0; b < NBR; ++b)
        if (b < nbr) {
          const GpBranch& g = (kTab ? tb[b] : a.br[b]).g;
          if (++pt[b] == g.g) { pt[b] = 0; ++pn[b]; pi[b] = 0; pj[b] = 0; }
          else if (++pj[b] == g.r) { pj[b] = 0; ++pi[b]; }
        }
    }
    // Every branch's loads are issued before any wait, with no exec-mask region around them: a
    // lane outside the branch's head group reads the group's first lane's o / lse (the same
    // cache lines, no extra traffic) and its weight is forced to zero below.  (Loads guarded by
    // `if (covered)` compiled to one wait per branch -- five serial memory latencies per token.)
    float lse[GP_MAX_BRANCHES];
    bool cov[GP_MAX_BRANCHES];
    uint2 ob[GP_MAX_BRANCHES][EPL / 4];
#pragma unroll
    for (int b = 0; b < NBR; ++b) {
      lse[b] = -1e8f;
      cov[b] = false;
      if (b < nbr) {
        const MergeBranch& mb = kTab ? tb[b] : a.br[b];
        const int lph = mb.g.hpg * (D / EPL);     // lanes per head group
        const int l0 = pj[b] * lph;
        cov[b] = lane >= l0 && lane < l0 + lph;
        const int ln = cov[b] ? lane : l0;
        const int64_t rb = (int64_t)(bidx * mb.g.nseg + pn[b]);
        lse[b] = mb.lse[(rb * a.H + ln * EPL / D) * mb.g.m + pi[b]];
        const uint2* src = reinterpret_cast<const uint2*>(mb.o + (rb * mb.g.m + pi[b]) * E + ln * EPL);
#pragma unroll
        for (int q = 0; q < EPL / 4; ++q) ob[b][q] = src[q];
      }
    }
    float wv[EPL], bv[EPL];
    if (a.ln_w != nullptr) {   // LN affine via L1, in flight with the o rows (-5 % vs loading after the sums)
      load_f32<EPL>(a.ln_w + col0, wv);
      load_f32<EPL>(a.ln_b + col0, bv);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int b = 0; b < NBR; ++b)
      if (b < nbr) {
        if (!cov[b] || lse[b] == 0.f) lse[b] = -1e8f;   // dilated_attention.py:46
        mx = fmaxf(mx, lse[b]);
      }
    float wsum = 0.f;
#pragma unroll
    for (int b = 0; b < NBR; ++b)
      if (b < nbr) {
        // v_exp_f32 / v_rcp_f32 (1 ulp) instead of the libm expf and the IEEE division sequence: the
        // weights are fp32 (the reference rounds them to the activation dtype, dilated_attention.py:128)
        lse[b] = fast_exp2((lse[b] - mx) * 1.44269504088896340736f);
        wsum += lse[b];
      }
    const float inv = __builtin_amdgcn_rcpf(wsum);
    float acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
#pragma unroll
    for (int b = 0; b < NBR; ++b) {
      if (b < nbr) {
        const float wb = cov[b] ? lse[b] * inv : 0.f;   // + 0 * finite leaves acc unchanged
#pragma unroll
        for (int q = 0; q < EPL / 4; ++q) {
          // explicit fma: every instantiation (and the varlen path) rounds identically
          acc[4 * q + 0] = __builtin_fmaf(e2f<kH>(ob[b][q].x), wb, acc[4 * q + 0]);
          acc[4 * q + 1] = __builtin_fmaf(e2f_hi<kH>(ob[b][q].x), wb, acc[4 * q + 1]);
          acc[4 * q + 2] = __builtin_fmaf(e2f<kH>(ob[b][q].y), wb, acc[4 * q + 2]);
          acc[4 * q + 3] = __builtin_fmaf(e2f_hi<kH>(ob[b][q].y), wb, acc[4 * q + 3]);
        }
      }
    }
    if (a.ln_w != nullptr) wave_layernorm_regs<EPL>(acc, E, wv, bv, a.eps);
    store_e<kH, EPL>(a.out + (int64_t)row * E + col0, acc);
  }
}

// ---------------------------------------------------------------------------------------
// Merge for E = 768, D = 48 (H = 16: every registered 768-wide arch, the product path), one token per
// wave as branch_merge_kernel, with fewer vector instructions per token (that kernel issues ~380 VALU
// per token-wave, ~70 of them 64-bit per-lane address arithmetic, and 12 dependent ds_bpermute for the
// LN sums):
//  * a lane owns two column chunks: 8 columns (one 16-byte access) and 4 columns (one 8-byte access)
//    instead of three 8-byte accesses of 12 contiguous columns: [8l, 8l + 8) of head l / 6 and
//    [512 + 4l, 516 + 4l) of head (128 + l) / 12 ("x8"), so each wave-instruction covers one contiguous span
//    (two heads per lane: twice the softmax VALU, yet measured faster than both chunks in one head, 81.3 vs
//    84.8 us per 70k launch, DESIGN §10: the kernel is bound by memory requests, not issue);
//  * loads address a wave-uniform row base plus a 32-bit lane offset (no per-lane 64-bit math);
//  * the LN row sums are xor-butterflies (DPP quad_perm / row_half_mirror / row_ror:8, then
//    v_permlane16/32_swap): the same sum in every lane, no LDS round trips.
// Per (token, head) the branch weights and the fp32 accumulation are branch_merge_kernel's bit for bit
// (dilated_attention.py:100-131).
// waves (tokens) per block of the v2 merge: consecutive tokens of one block share their lse / o lines in L1
#ifndef GP_MERGE_WPB
#define GP_MERGE_WPB 4
#endif

// A 32-bit lane offset the compiler may not re-associate with constants: keeps a uniform-base + lane-offset
// load in its SGPR-base (saddr) form instead of a per-lane 64-bit address.
GP_DEV uint32_t opaque_u32(uint32_t x) {
  __asm__("" : "+v"(x));
  return x;
}

GP_DEV float wave_sum_xor(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));   // quad_perm 1,0,3,2
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));   // quad_perm 2,3,0,1
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));  // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));  // row_ror:8
  const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
  const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
}

template <int NBR, bool kTab, bool kH>
__global__ __launch_bounds__(64 * GP_MERGE_WPB) void branch_merge_v2_kernel(const MergeArgs a) {
  // no implicit contraction: the compiler fused v - s * (1/E) into one fma in some instantiations only, so the
  // packed (varlen) and single-slide merges differed in the last bit; every fma below is explicit
#pragma clang fp contract(off)
  constexpr int E = 768, H = 16, D = 48;
  const int nbr = NBR < GP_MAX_BRANCHES ? NBR : a.nbranch;
  const int lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane((int)blockIdx.x * GP_MERGE_WPB + (int)(threadIdx.x >> 6));
  const int total = (int)(a.B * a.ntok);
  if (row >= total) return;
  // the lane's chunks: columns c0 .. c0 + 7 (head h0) and c1 .. c1 + 3 (head h1)
  const int h0 = lane / 6;
  const int h1 = (128 + lane) / 12;
  const int c0 = 8 * lane;
  const int c1 = 512 + 4 * lane;
  // LN affine (L1-resident): issued with the branch loads; nothing is read without an LN (a null ln_w)
  const bool ln = a.ln_w != nullptr;
  float w0[8] = {}, w1[4] = {}, b0[8] = {}, b1[4] = {};
  if (ln) {
    load_f32<8>(a.ln_w + c0, w0);
    load_f32<4>(a.ln_w + c1, w1);
    load_f32<8>(a.ln_b + c0, b0);
    load_f32<4>(a.ln_b + c1, b1);
  }
  int bidx = 0, p;
  MergeBranch tb[kTab ? GP_MAX_BRANCHES : 1];
  if constexpr (kTab) {
    int lo = 0, hi = a.nslide - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((int64_t)row >= a.tok_off[mid]) lo = mid; else hi = mid - 1;
    }
    p = (int)(row - a.tok_off[lo]);
#pragma unroll
    for (int b = 0; b < NBR; ++b)
      if (b < nbr) tb[b] = a.mtab[lo * a.nbranch + b];
  } else {
    bidx = (int)div_magic((uint32_t)row, a.dnt);
    p = (int)a.tok_lo + (row - bidx * (int)a.ntok);
  }
  // every branch's loads before any wait; a lane outside the branch's head group reads the group's
  // first head (same cache lines as the covered lanes) and gets weight 0
  uint4 o0[NBR];
  uint2 o1[NBR];
  float l0[NBR], l1[NBR];
  bool cv0[NBR], cv1[NBR];
#pragma unroll
  for (int b = 0; b < NBR; ++b) {
    cv0[b] = cv1[b] = false;
    l0[b] = l1[b] = -1e8f;
    o0[b] = make_uint4(0, 0, 0, 0);
    o1[b] = make_uint2(0, 0);
    if (b < nbr) {
      const MergeBranch& mb = kTab ? tb[b] : a.br[b];
      const int pn = (int)div_magic((uint32_t)p, mb.dg);
      const int pt = p - pn * mb.g.g;
      const int pi = (int)div_magic((uint32_t)pt, mb.dr);
      const int pj = pt - pi * mb.g.r;
      const int hpg = mb.g.hpg;
      const int hf = pj * hpg;                                 // the covered group's first head
      // 32-bit byte offsets: the launch checks every branch's o / lse buffer is below 4 GiB
      const uint32_t rb = (uint32_t)(bidx * mb.g.nseg + pn);
      const char* orow = reinterpret_cast<const char*>(mb.o) + (rb * (uint32_t)mb.g.m + (uint32_t)pi) * (uint32_t)(E * 2);
      const char* lrow = reinterpret_cast<const char*>(mb.lse) + (rb * (uint32_t)(H * mb.g.m) + (uint32_t)pi) * 4u;
      const uint32_t m4 = (uint32_t)mb.g.m * 4u;
      cv0[b] = (unsigned)(h0 - hf) < (unsigned)hpg;
      const int s0 = cv0[b] ? h0 : hf;
      // (m < 2^22 for any segment of the schedule: 24-bit multiplies)
      l0[b] = *reinterpret_cast<const float*>(lrow + opaque_u32(__umul24((uint32_t)s0, m4)));
      cv1[b] = (unsigned)(h1 - hf) < (unsigned)hpg;
      l1[b] = *reinterpret_cast<const float*>(lrow + opaque_u32(__umul24((uint32_t)(cv1[b] ? h1 : hf), m4)));
      o0[b] = *reinterpret_cast<const uint4*>(orow + opaque_u32(cv0[b] ? 2 * c0 : 2 * D * hf));
      o1[b] = *reinterpret_cast<const uint2*>(orow + opaque_u32(cv1[b] ? 2 * c1 : 2 * D * hf));
    }
  }
  // per-head softmax over the branches
  float mx0 = -INFINITY, mx1 = -INFINITY;
#pragma unroll
  for (int b = 0; b < NBR; ++b)
    if (b < nbr) {
      if (!cv0[b] || l0[b] == 0.f) l0[b] = -1e8f;   // dilated_attention.py:46
      mx0 = fmaxf(mx0, l0[b]);
      if (!cv1[b] || l1[b] == 0.f) l1[b] = -1e8f;
      mx1 = fmaxf(mx1, l1[b]);
    }
  float ws0 = 0.f, ws1 = 0.f;
#pragma unroll
  for (int b = 0; b < NBR; ++b)
    if (b < nbr) {
      l0[b] = fast_exp2((l0[b] - mx0) * 1.44269504088896340736f);
      ws0 += l0[b];
      l1[b] = fast_exp2((l1[b] - mx1) * 1.44269504088896340736f);
      ws1 += l1[b];
    }
  const float inv0 = __builtin_amdgcn_rcpf(ws0), inv1 = __builtin_amdgcn_rcpf(ws1);
  float v[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) v[e] = 0.f;
#pragma unroll
  for (int b = 0; b < NBR; ++b)
    if (b < nbr) {
      const float wb0 = cv0[b] ? l0[b] * inv0 : 0.f;   // + 0 * finite leaves v unchanged
      const float wb1 = cv1[b] ? l1[b] * inv1 : 0.f;
      const uint32_t u0[4] = {o0[b].x, o0[b].y, o0[b].z, o0[b].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[2 * k] = __builtin_fmaf(e2f<kH>(u0[k]), wb0, v[2 * k]);
        v[2 * k + 1] = __builtin_fmaf(e2f_hi<kH>(u0[k]), wb0, v[2 * k + 1]);
      }
      v[8] = __builtin_fmaf(e2f<kH>(o1[b].x), wb1, v[8]);
      v[9] = __builtin_fmaf(e2f_hi<kH>(o1[b].x), wb1, v[9]);
      v[10] = __builtin_fmaf(e2f<kH>(o1[b].y), wb1, v[10]);
      v[11] = __builtin_fmaf(e2f_hi<kH>(o1[b].y), wb1, v[11]);
    }
  if (ln) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 12; ++e) s += v[e];
    const float mean = wave_sum_xor(s) * (1.0f / E);
    // explicit fmas: every instantiation (the varlen one included) rounds the LN identically
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      const float d = v[e] - mean;
      q = __builtin_fmaf(d, d, q);
    }
    const float rstd = rsqrtf(__builtin_fmaf(wave_sum_xor(q), 1.0f / E, a.eps));
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaf((v[e] - mean) * rstd, w0[e], b0[e]);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[8 + e] = __builtin_fmaf((v[8 + e] - mean) * rstd, w1[e], b1[e]);
  }
  char* orow = reinterpret_cast<char*>(a.out) + (int64_t)row * (E * 2);
  *reinterpret_cast<uint4*>(orow + 2 * c0) =
      make_uint4(pack2e<kH>(v[0], v[1]), pack2e<kH>(v[2], v[3]), pack2e<kH>(v[4], v[5]), pack2e<kH>(v[6], v[7]));
  *reinterpret_cast<uint2*>(orow + 2 * c1) = make_uint2(pack2e<kH>(v[8], v[9]), pack2e<kH>(v[10], v[11]));
}

// v3 (round 6, the product merge): the v2 merge with the LSEs staged per block of up to kV3Tok consecutive tokens.  The
// [B * nseg, H, m] lse layout puts one token's covered heads in 16 / r different cache lines, and the v2 kernel's
// one-token waves fetch them token by token (~16 of its ~42 L2 read requests per token, at the per-CU cap of
// outstanding requests, §3.5).  Here the block's four waves first load every lse its 64 tokens need -- lane t =
// token t, so one wave-instruction reads up to 64 consecutive rows of a head -- into LDS, then each wave merges
// a quarter of the tokens (t = wave + 4k) exactly as branch_merge_v2_kernel does, reading the weights' LSEs from
// LDS.  Same arithmetic per token, so the same bits (the varlen merge too).  Same-process A/B
// (profiles/r06_mv3e_merge_ab_*): 70k 73.5 vs 84.2 us, 256k 238 vs 284 us per launch, bit-identical; up to 64
// tokens per block 82.5 / 246 us, 16: 82.0 / 272 us.  The packed-slide (varlen) merge runs on it too, when every
// slide holds at least a block's tokens: C5 batch (675,619 tokens) 0.625 vs 0.868 ms per launch, bit-identical
// (profiles/r06_mv3tab2_*)
#ifndef GP_MERGE_V3_TOK
#define GP_MERGE_V3_TOK 32
#endif
constexpr int kV3Tok = GP_MERGE_V3_TOK;    // most tokens per block (4 waves, up to kV3Tok / 4 tokens each); <= 64

// entry k of the token list, held inside [0, L): a bad list cannot send a load outside the branch buffers
GP_DEV int list_token(const MergeArgs& a, int k) {
  const int p = a.tok_list[k];
  return p < 0 ? 0 : (p < (int)a.L ? p : (int)a.L - 1);
}

// A MergeBranch table entry by scalar loads (uniform index, constant address space): the entries then live in
// SGPRs even when the load follows the kernel's global stores (the compiler's uniform-load analysis would
// otherwise fall back to per-lane loads into VGPRs)
GP_DEV MergeBranch merge_entry_scalar(const MergeBranch* tab, int idx) {
  MergeBranch e;
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert(sizeof(MergeBranch) % 4 == 0, "");
  uint32_t words[sizeof(MergeBranch) / 4];
  const __attribute__((address_space(4))) uint32_t* src =
      (const __attribute__((address_space(4))) uint32_t*)(uintptr_t)(tab + __builtin_amdgcn_readfirstlane(idx));
#pragma unroll
  for (int i = 0; i < (int)(sizeof(MergeBranch) / 4); ++i) words[i] = src[i];
  __builtin_memcpy(&e, words, sizeof(MergeBranch));
#else
  e = tab[idx];
#endif
  return e;
}

// kList (gp_branch_merge_ln_rows): output row b*ntok + k merges token tok_list[k] of batch b instead of token
// tok_lo + k -- the only difference, so a listed token's row holds the bits the full merge writes for it.
template <int NBR, bool kH, bool kTab = false, bool kList = false>
__global__ __launch_bounds__(256) void branch_merge_v3_kernel(const MergeArgs a, const int tpb) {
#pragma clang fp contract(off)
  static_assert(!(kTab && kList), "token list: [B, L] batches only");
  constexpr int E = 768, H = 16, D = 48;
  constexpr int LS = NBR * 16 + 1;           // LDS floats per token (16 per branch entry; +1: bank spread)
  __shared__ float lse_s[kV3Tok * LS];
  const int nbr = NBR < GP_MAX_BRANCHES ? NBR : a.nbranch;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int total = (int)(a.B * a.ntok);
  const int row0 = (int)blockIdx.x * tpb;    // tpb <= kV3Tok tokens of this block (the launch balances them)
  // kTab (packed slides): the slide of the block's first token (wave-uniform binary search); a block of at most
  // kV3Tok tokens meets at most two slides (every slide holds more tokens than that, checked by the launch)
  int slide0 = 0;
  if constexpr (kTab) {
    int lo = 0, hi = a.nslide - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((int64_t)row0 >= a.tok_off[mid]) lo = mid; else hi = mid - 1;
    }
    slide0 = __builtin_amdgcn_readfirstlane(lo);
  }
  // ---- stage: lane t loads, for token row0 + t, the covered heads' lse of every branch (wave w: heads h' = w mod 4)
  if constexpr (!kTab) {
    if (lane < tpb) {
      const int tl = lane;
      const int row = row0 + tl;
      const bool live = row < total;
      const int rr = live ? row : total - 1;
      const int bidx = (int)div_magic((uint32_t)rr, a.dnt);
      const int p = kList ? list_token(a, rr - bidx * (int)a.ntok) : (int)a.tok_lo + (rr - bidx * (int)a.ntok);
#pragma unroll
      for (int b = 0; b < NBR; ++b) {
        if (b < nbr) {
          const MergeBranch& mb = a.br[b];
          const int pn = (int)div_magic((uint32_t)p, mb.dg);
          const int pt = p - pn * mb.g.g;
          const int pi = (int)div_magic((uint32_t)pt, mb.dr);
          const int pj = pt - pi * mb.g.r;
          const int hpg = mb.g.hpg;
          const uint32_t rb = (uint32_t)(bidx * mb.g.nseg + pn);
          const float* lrow = mb.lse + (size_t)rb * (uint32_t)(H * mb.g.m) + (uint32_t)pi;
          for (int hq = wv; hq < hpg; hq += 4) {
            const float v = lrow[(size_t)(uint32_t)(pj * hpg + hq) * (uint32_t)mb.g.m];
            lse_s[tl * LS + b * 16 + hq] = v;
          }
        }
      }
    }
  } else {
#pragma unroll
    for (int pass = 0; pass < (kTab ? 2 : 1); ++pass) {
      int s_lo = 0, s_hi = total;
      MergeBranch tb[kTab ? NBR : 1];
      if constexpr (kTab) {
        const int sl = slide0 + pass;
        if (sl >= a.nslide) break;
        s_lo = (int)a.tok_off[sl];
        s_hi = (int)a.tok_off[sl + 1];
#pragma unroll
        for (int b = 0; b < NBR; ++b)
          if (b < nbr) tb[b] = a.mtab[sl * a.nbranch + b];
      }
      const int tl = lane;
      const int row = row0 + tl;
      if (tl < tpb && row < total && row >= s_lo && row < s_hi) {
        int bidx = 0, p;
        if constexpr (kTab) {
          p = row - s_lo;
        } else {
          bidx = (int)div_magic((uint32_t)row, a.dnt);
          p = (int)a.tok_lo + (row - bidx * (int)a.ntok);
        }
#pragma unroll
        for (int b = 0; b < NBR; ++b) {
          if (b < nbr) {
            const MergeBranch& mb = kTab ? tb[b] : a.br[b];
            const int pn = (int)div_magic((uint32_t)p, mb.dg);
            const int pt = p - pn * mb.g.g;
            const int pi = (int)div_magic((uint32_t)pt, mb.dr);
            const int pj = pt - pi * mb.g.r;
            const int hpg = mb.g.hpg;
            const uint32_t rb = (uint32_t)(bidx * mb.g.nseg + pn);
            const float* lrow = mb.lse + (size_t)rb * (uint32_t)(H * mb.g.m) + (uint32_t)pi;
            for (int hq = wv; hq < hpg; hq += 4) {
              const float v = lrow[(size_t)(uint32_t)(pj * hpg + hq) * (uint32_t)mb.g.m];
              lse_s[tl * LS + b * 16 + hq] = v;
            }
          }
        }
      }
    }
  }
  __syncthreads();
  // ---- merge: wave wv takes tokens wv, wv + 4, ..., as branch_merge_v2_kernel does one token
  const int kq = lane & 3;
  (void)kq;
  const int h0 = lane / 6, h1 = (128 + lane) / 12;
  const int c0 = 8 * lane, c1 = 512 + 4 * lane;
  const bool ln = a.ln_w != nullptr;
  float w0[8] = {}, w1[4] = {}, b0[8] = {}, b1[4] = {};
  if (ln) {                                  // (without an LN nothing is read: the output may be a small buffer)
    load_f32<8>(a.ln_w + c0, w0);
    load_f32<4>(a.ln_w + c1, w1);
    load_f32<8>(a.ln_b + c0, b0);
    load_f32<4>(a.ln_b + c1, b1);
  }
  // kTab: the first slide's entries, loaded once for the wave's tokens (its tokens ascend, so a crossing into
  // the next slide happens at most once)
  MergeBranch tb[kTab ? NBR : 1];
  int t_sl = 0, t_base = 0, t_bnd = INT_MAX;
  if constexpr (kTab) {
    t_sl = slide0;
    t_base = (int)a.tok_off[slide0];
    t_bnd = slide0 + 1 < a.nslide ? (int)a.tok_off[slide0 + 1] : INT_MAX;
#pragma unroll
    for (int b = 0; b < NBR; ++b)
      if (b < nbr) tb[b] = merge_entry_scalar(a.mtab, slide0 * a.nbranch + b);
  }
  for (int k = 0; k < kV3Tok / 4; ++k) {
    const int t = wv + 4 * k;
    const int row = row0 + t;
    if (t >= tpb || row >= total) break;
    int bidx = 0, p;
    if constexpr (kTab) {
      if (row >= t_bnd) {                    // this wave's tokens crossed into the next slide (rare): switch tables
        t_sl += 1;
        t_base = t_bnd;
        t_bnd = t_sl + 1 < a.nslide ? (int)a.tok_off[t_sl + 1] : INT_MAX;
#pragma unroll
        for (int b = 0; b < NBR; ++b)
          if (b < nbr) tb[b] = merge_entry_scalar(a.mtab, t_sl * a.nbranch + b);
      }
      p = row - t_base;
    } else {
      bidx = (int)div_magic((uint32_t)row, a.dnt);
      p = kList ? list_token(a, row - bidx * (int)a.ntok) : (int)a.tok_lo + (row - bidx * (int)a.ntok);
    }
    uint4 o0[NBR];
    uint2 o1[NBR];
    float l0[NBR], l1[NBR];
    bool cv0[NBR], cv1[NBR];
#pragma unroll
    for (int b = 0; b < NBR; ++b) {
      cv0[b] = cv1[b] = false;
      l0[b] = l1[b] = -1e8f;
      o0[b] = make_uint4(0, 0, 0, 0);
      o1[b] = make_uint2(0, 0);
      if (b < nbr) {
        const MergeBranch& mb = kTab ? tb[b] : a.br[b];
        const int pn = (int)div_magic((uint32_t)p, mb.dg);
        const int pt = p - pn * mb.g.g;
        const int pi = (int)div_magic((uint32_t)pt, mb.dr);
        const int pj = pt - pi * mb.g.r;
        const int hpg = mb.g.hpg;
        const int hf = pj * hpg;
        const uint32_t rb = (uint32_t)(bidx * mb.g.nseg + pn);
        const char* orow = reinterpret_cast<const char*>(mb.o) + (rb * (uint32_t)mb.g.m + (uint32_t)pi) * (uint32_t)(E * 2);
        cv0[b] = (unsigned)(h0 - hf) < (unsigned)hpg;
        cv1[b] = (unsigned)(h1 - hf) < (unsigned)hpg;
        l0[b] = lse_s[t * LS + b * 16 + (cv0[b] ? h0 - hf : 0)];
        l1[b] = lse_s[t * LS + b * 16 + (cv1[b] ? h1 - hf : 0)];
        o0[b] = *reinterpret_cast<const uint4*>(orow + opaque_u32(cv0[b] ? 2 * c0 : 2 * D * hf));
        o1[b] = *reinterpret_cast<const uint2*>(orow + opaque_u32(cv1[b] ? 2 * c1 : 2 * D * hf));
      }
    }
    float mx0 = -INFINITY, mx1 = -INFINITY;
#pragma unroll
    for (int b = 0; b < NBR; ++b)
      if (b < nbr) {
        if (!cv0[b] || l0[b] == 0.f) l0[b] = -1e8f;   // dilated_attention.py:46
        mx0 = fmaxf(mx0, l0[b]);
        if (!cv1[b] || l1[b] == 0.f) l1[b] = -1e8f;
        mx1 = fmaxf(mx1, l1[b]);
      }
    float ws0 = 0.f, ws1 = 0.f;
#pragma unroll
    for (int b = 0; b < NBR; ++b)
      if (b < nbr) {
        l0[b] = fast_exp2((l0[b] - mx0) * 1.44269504088896340736f);
        ws0 += l0[b];
        l1[b] = fast_exp2((l1[b] - mx1) * 1.44269504088896340736f);
        ws1 += l1[b];
      }
    const float inv0 = __builtin_amdgcn_rcpf(ws0), inv1 = __builtin_amdgcn_rcpf(ws1);
    float v[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) v[e] = 0.f;
#pragma unroll
    for (int b = 0; b < NBR; ++b)
      if (b < nbr) {
        const float wb0 = cv0[b] ? l0[b] * inv0 : 0.f;
        const float wb1 = cv1[b] ? l1[b] * inv1 : 0.f;
        const uint32_t u0[4] = {o0[b].x, o0[b].y, o0[b].z, o0[b].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          v[2 * q] = __builtin_fmaf(e2f<kH>(u0[q]), wb0, v[2 * q]);
          v[2 * q + 1] = __builtin_fmaf(e2f_hi<kH>(u0[q]), wb0, v[2 * q + 1]);
        }
        v[8] = __builtin_fmaf(e2f<kH>(o1[b].x), wb1, v[8]);
        v[9] = __builtin_fmaf(e2f_hi<kH>(o1[b].x), wb1, v[9]);
        v[10] = __builtin_fmaf(e2f<kH>(o1[b].y), wb1, v[10]);
        v[11] = __builtin_fmaf(e2f_hi<kH>(o1[b].y), wb1, v[11]);
      }
    if (ln) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 12; ++e) s += v[e];
      const float mean = wave_sum_xor(s) * (1.0f / E);
      float q = 0.f;
#pragma unroll
      for (int e = 0; e < 12; ++e) {
        const float d = v[e] - mean;
        q = __builtin_fmaf(d, d, q);
      }
      const float rstd = rsqrtf(__builtin_fmaf(wave_sum_xor(q), 1.0f / E, a.eps));
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaf((v[e] - mean) * rstd, w0[e], b0[e]);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[8 + e] = __builtin_fmaf((v[8 + e] - mean) * rstd, w1[e], b1[e]);
    }
    char* orow = reinterpret_cast<char*>(a.out) + (int64_t)row * (E * 2);
    *reinterpret_cast<uint4*>(orow + 2 * c0) =
        make_uint4(pack2e<kH>(v[0], v[1]), pack2e<kH>(v[2], v[3]), pack2e<kH>(v[4], v[5]), pack2e<kH>(v[6], v[7]));
    *reinterpret_cast<uint2*>(orow + 2 * c1) = make_uint2(pack2e<kH>(v[8], v[9]), pack2e<kH>(v[10], v[11]));
  }
}

// ---------------------------------------------------------------------------------------
// the E = 768 / D = 48 merge: one token per wave, 4 waves per block
unsigned merge_v2_grid(int64_t tokens) { return (unsigned)((tokens + GP_MERGE_WPB - 1) / GP_MERGE_WPB); }
// its 32-bit byte offsets: every branch's o rows (B * nseg * m rows of 1,536 B) below 4 GiB
bool merge_v2_fits(const MergeArgs& a) {
  for (int b = 0; b < a.nbranch; ++b)
    if ((uint64_t)a.B * a.br[b].g.nseg * a.br[b].g.m * 1536u >= (1ull << 32)) return false;
  return true;
}

// The v3 merge's tokens per block and grid for T tokens: the blocks spread evenly over the CUs -- the kernel is
// bound per CU (outstanding L2 requests), so a CU holding one block more than another finishes a block's time
// later (70k: 9 blocks of 31 tokens per CU; 256k: 32 blocks of 32)
struct MergeV3Shape {
  int tpb;
  unsigned grid;
};
MergeV3Shape merge_v3_launch_shape(int64_t T, int64_t ncu) {
  const int64_t per_cu = (T + ncu * kV3Tok - 1) / (ncu * kV3Tok);
  const int tpb = (int)std::max<int64_t>(1, (T + ncu * per_cu - 1) / (ncu * per_cu));
  return {tpb, (unsigned)((T + tpb - 1) / tpb)};
}

template <bool kH>
void launch_merge(const MergeArgs& a, int E, int D, int nbranch, unsigned nb, hipStream_t s) {
  switch (E) {
    case 768:
      // (5 entries only: the 7 / 8-entry instantiations need 134-145 VGPRs and spill SGPRs; they keep the v2 kernel)
      if (D == 48 && nbranch == 5 && merge_v2_fits(a)) {
        const MergeV3Shape sh = merge_v3_launch_shape(a.B * a.ntok, attn_num_cus(s));
        branch_merge_v3_kernel<5, kH><<<sh.grid, 256, 0, s>>>(a, sh.tpb);
      } else if (D == 48 && merge_v2_fits(a)) {
        const unsigned g = merge_v2_grid(a.B * a.ntok);
        // (5 branches, two of them in two key parts: the sequence-parallel long-branch split, seqpar.plan_key_parts)
        if (nbranch == 7) branch_merge_v2_kernel<7, false, kH><<<g, 64 * GP_MERGE_WPB, 0, s>>>(a);
        else branch_merge_v2_kernel<GP_MAX_BRANCHES, false, kH><<<g, 64 * GP_MERGE_WPB, 0, s>>>(a);
      } else if (D == 96) branch_merge_kernel<12, 96, false, GP_MAX_BRANCHES, kH><<<nb, 256, 0, s>>>(a);
      else branch_merge_kernel<12, 12, false, GP_MAX_BRANCHES, kH><<<nb, 256, 0, s>>>(a);
      break;
    case 1024:
      if (D == 64) branch_merge_kernel<16, 64, false, GP_MAX_BRANCHES, kH><<<nb, 256, 0, s>>>(a);
      else branch_merge_kernel<16, 16, false, GP_MAX_BRANCHES, kH><<<nb, 256, 0, s>>>(a);
      break;
    case 1536:
      if (D == 96) branch_merge_kernel<24, 96, false, GP_MAX_BRANCHES, kH><<<nb, 256, 0, s>>>(a);
      else if (D == 48) branch_merge_kernel<24, 48, false, GP_MAX_BRANCHES, kH><<<nb, 256, 0, s>>>(a);
      else branch_merge_kernel<24, 24, false, GP_MAX_BRANCHES, kH><<<nb, 256, 0, s>>>(a);
      break;
  }
}

// The launch arguments of a [B, L] merge (the callers have checked theirs): tokens [tok_lo, tok_lo + n_tok) of
// every batch, or the n_tok listed tokens tok_list
void fill_merge_args(MergeArgs& a, const uint16_t* const* o_in, const float* const* lse_in, const int32_t* seg_len,
                     const int32_t* ratios, int nbranch, int64_t B, int64_t L, int64_t tok_lo, int64_t n_tok,
                     const int32_t* tok_list, int H, int D, const float* ln_w, const float* ln_b, float eps,
                     uint16_t* out) {
  a.B = B; a.L = L; a.H = H; a.D = D; a.E = H * D; a.nbranch = nbranch;
  a.tok_lo = tok_lo; a.ntok = n_tok;
  a.dnt = make_div_magic((uint32_t)n_tok);
  a.tok_list = tok_list;
  for (int b = 0; b < nbranch; ++b) {
    a.br[b].g = gp_make_branch(L, seg_len[b], ratios[b], H);
    a.br[b].o = o_in[b];
    a.br[b].lse = lse_in[b];
    merge_branch_magic(a.br[b]);
  }
  for (int b = nbranch; b < GP_MAX_BRANCHES; ++b) a.br[b] = a.br[nbranch - 1];
  a.ln_w = ln_w; a.ln_b = ln_b; a.eps = eps; a.out = out;
  a.mtab = nullptr; a.tok_off = nullptr; a.nslide = 0;
}

}  // namespace

// =========================================================================================
extern "C" int gp_branch_merge_ln(const uint16_t* const* o_in, const float* const* lse_in, const int32_t* seg_len,
                                  const int32_t* ratios, int nbranch, int64_t B, int64_t L, int H, int D,
                                  const float* ln_w, const float* ln_b, float eps, uint16_t* out, int fmt,
                                  void* stream) {
  return gp_branch_merge_ln_window(o_in, lse_in, seg_len, ratios, nbranch, B, L, 0, L, H, D, ln_w, ln_b, eps, out,
                                   fmt, stream);
}

extern "C" int gp_branch_merge_ln_window(const uint16_t* const* o_in, const float* const* lse_in,
                                         const int32_t* seg_len, const int32_t* ratios, int nbranch, int64_t B,
                                         int64_t L, int64_t tok_lo, int64_t n_tok, int H, int D, const float* ln_w,
                                         const float* ln_b, float eps, uint16_t* out, int fmt, void* stream) {
  const int E = H * D;
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16, "gp_branch_merge_ln: bad fmt %d", fmt);
  GP_REQUIRE(nbranch >= 1 && nbranch <= GP_MAX_BRANCHES, "gp_branch_merge_ln: nbranch must be 1..%d", GP_MAX_BRANCHES);
  GP_REQUIRE((E == 768 && (D == 48 || D == 96 || D == 12)) || (E == 1024 && (D == 64 || D == 16)) ||
                 (E == 1536 && (D == 96 || D == 48 || D == 24)),
             "gp_branch_merge_ln: H*D=%d with D=%d unsupported", E, D);
  GP_REQUIRE(B * L < (int64_t)0x7fffffff, "gp_branch_merge_ln: B*L too large");
  GP_REQUIRE(B > 0 && L > 0 && tok_lo >= 0 && n_tok >= 0 && tok_lo + n_tok <= L, "gp_branch_merge_ln: bad sizes");
  if (n_tok == 0) return 0;
  GP_REQUIRE(o_in && lse_in && seg_len && ratios && out, "gp_branch_merge_ln: null pointer");
  GP_REQUIRE(ln_w == nullptr || ln_b != nullptr, "gp_branch_merge_ln: ln_w without ln_b");
  for (int b = 0; b < nbranch; ++b)
    GP_REQUIRE(seg_len[b] > 0 && ratios[b] > 0 && o_in[b] && lse_in[b], "gp_branch_merge_ln: bad branch %d", b);
  MergeArgs a;
  fill_merge_args(a, o_in, lse_in, seg_len, ratios, nbranch, B, L, tok_lo, n_tok, nullptr, H, D, ln_w, ln_b, eps, out);
  const unsigned nb = (unsigned)((B * n_tok + 4 * kTPW - 1) / (4 * kTPW));   // kTPW tokens per wave
  if (fmt == GP_FMT_F16) launch_merge<true>(a, E, D, nbranch, nb, gp_stream(stream));
  else launch_merge<false>(a, E, D, nbranch, nb, gp_stream(stream));
  return gp_check_launch("gp_branch_merge_ln");
}

// the listed-token merge runs on branch_merge_v3_kernel alone: E = 768, D = 48, five branch entries
extern "C" int gp_branch_merge_ln_rows_supported(int H, int D, int nbranch) {
  return H == 16 && D == 48 && nbranch == 5;
}

extern "C" int gp_branch_merge_ln_rows(const uint16_t* const* o_in, const float* const* lse_in,
                                       const int32_t* seg_len, const int32_t* ratios, int nbranch, int64_t B,
                                       int64_t L, const int32_t* rows, int64_t n_rows, int H, int D,
                                       const float* ln_w, const float* ln_b, float eps, uint16_t* out, int fmt,
                                       void* stream) {
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16, "gp_branch_merge_ln_rows: bad fmt %d", fmt);
  GP_REQUIRE(gp_branch_merge_ln_rows_supported(H, D, nbranch),
             "gp_branch_merge_ln_rows: H %d, D %d, %d branches unsupported (16, 48, 5)", H, D, nbranch);
  GP_REQUIRE(B * L < (int64_t)0x7fffffff, "gp_branch_merge_ln_rows: B*L too large");
  GP_REQUIRE(B > 0 && L > 0 && n_rows >= 0 && n_rows <= L, "gp_branch_merge_ln_rows: bad sizes");
  if (n_rows == 0) return 0;
  GP_REQUIRE(o_in && lse_in && seg_len && ratios && rows && out, "gp_branch_merge_ln_rows: null pointer");
  GP_REQUIRE(ln_w == nullptr || ln_b != nullptr, "gp_branch_merge_ln_rows: ln_w without ln_b");
  GP_REQUIRE(gp_aligned(out, 16), "gp_branch_merge_ln_rows: out must be 16-byte aligned");
  for (int b = 0; b < nbranch; ++b)
    GP_REQUIRE(seg_len[b] > 0 && ratios[b] > 0 && o_in[b] && lse_in[b], "gp_branch_merge_ln_rows: bad branch %d", b);
  MergeArgs a;
  fill_merge_args(a, o_in, lse_in, seg_len, ratios, nbranch, B, L, 0, n_rows, rows, H, D, ln_w, ln_b, eps, out);
  GP_REQUIRE(merge_v2_fits(a), "gp_branch_merge_ln_rows: a branch's o rows pass 4 GiB");
  hipStream_t s = gp_stream(stream);
  const MergeV3Shape sh = merge_v3_launch_shape(B * n_rows, attn_num_cus(s));
  if (fmt == GP_FMT_F16) branch_merge_v3_kernel<5, true, false, true><<<sh.grid, 256, 0, s>>>(a, sh.tpb);
  else branch_merge_v3_kernel<5, false, false, true><<<sh.grid, 256, 0, s>>>(a, sh.tpb);
  return gp_check_launch("gp_branch_merge_ln_rows");
}

// the packed-slide (varlen) merge: the plan is gp_varlen_plan's (gp_attn.hip; layout in gp_attn_plan.h)
extern "C" int gp_branch_merge_ln_varlen(const void* plan_host, const void* plan_dev, const float* ln_w,
                                         const float* ln_b, float eps, uint16_t* out, int fmt, void* stream) {
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16, "gp_branch_merge_ln_varlen: bad fmt %d", fmt);
  GP_REQUIRE(plan_host && plan_dev && gp_aligned(plan_dev, 16), "gp_branch_merge_ln_varlen: null/misaligned plan");
  const VarlenHdr h = *static_cast<const VarlenHdr*>(plan_host);
  GP_REQUIRE(h.magic == kVarlenMagic, "gp_branch_merge_ln_varlen: not a gp_varlen_plan buffer");
  GP_REQUIRE(h.H * h.D == 768 && h.D == 48, "gp_branch_merge_ln_varlen: needs H*D = 768, D = 48");
  GP_REQUIRE(out && (ln_w == nullptr || ln_b != nullptr), "gp_branch_merge_ln_varlen: bad output / LN arguments");
  MergeArgs a;
  memset(&a, 0, sizeof(a));
  a.B = 1; a.L = h.T; a.tok_lo = 0; a.ntok = h.T;
  a.H = h.H; a.D = h.D; a.E = h.H * h.D; a.nbranch = h.nbranch;
  a.ln_w = ln_w; a.ln_b = ln_b; a.eps = eps; a.out = out;
  a.mtab = reinterpret_cast<const MergeBranch*>(static_cast<const char*>(plan_dev) + h.mtab_off);
  a.tok_off = reinterpret_cast<const int64_t*>(static_cast<const char*>(plan_dev) + h.tok_off_off);
  a.nslide = h.nslide;
  // (the v2 kernel's 32-bit offsets run from each slide's own o / lse region: a slide's branch rows
  // are at most 2 L_i, below 4 GiB for any slide the 1000 x 1000 position grid admits)
  const unsigned nb = merge_v2_grid(h.T);
  hipStream_t s = gp_stream(stream);
  if (h.nbranch == 5) {
    // the v3 merge over the packed tokens when every slide holds at least a block's tokens (a block then meets at
    // most two slides); tokens per block as the single-slide launch
    const int64_t* toh = reinterpret_cast<const int64_t*>(static_cast<const char*>(plan_host) + h.tok_off_off);
    int64_t shortest = INT64_MAX;
    for (int i = 0; i < h.nslide; ++i) shortest = std::min<int64_t>(shortest, toh[i + 1] - toh[i]);
    const MergeV3Shape sh = merge_v3_launch_shape(h.T, attn_num_cus(s));
    if (shortest >= sh.tpb) {
      if (fmt == GP_FMT_F16) branch_merge_v3_kernel<5, true, true><<<sh.grid, 256, 0, s>>>(a, sh.tpb);
      else branch_merge_v3_kernel<5, false, true><<<sh.grid, 256, 0, s>>>(a, sh.tpb);
      return gp_check_launch("gp_branch_merge_ln_varlen");
    }
  }
  if (h.nbranch == 5) {   // every registered arch's schedule: compile-time branch loops
    if (fmt == GP_FMT_F16) branch_merge_v2_kernel<5, true, true><<<nb, 64 * GP_MERGE_WPB, 0, s>>>(a);
    else branch_merge_v2_kernel<5, true, false><<<nb, 64 * GP_MERGE_WPB, 0, s>>>(a);
  } else if (fmt == GP_FMT_F16) {
    branch_merge_v2_kernel<GP_MAX_BRANCHES, true, true><<<nb, 64 * GP_MERGE_WPB, 0, s>>>(a);
  } else {
    branch_merge_v2_kernel<GP_MAX_BRANCHES, true, false><<<nb, 64 * GP_MERGE_WPB, 0, s>>>(a);
  }
  return gp_check_launch("gp_branch_merge_ln_varlen");
}
