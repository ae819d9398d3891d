// Weight gradient of nn.Linear on gfx950 MFMAs, with the bias gradient from the same pass over dY
// (gp_linear_wgrad): the backward of the QKV / out-proj / fc1 / fc2 / patch projections of the training path
// (multihead_attention.py:43-48, feedforward_network.py:131-142, slide_encoder.py:47-51).
//
//   dW[n, k] = sum_{m < M} dY[m, n] X[m, k]      fp32 [N, ldw]
//   db[n]    = sum_{m < M} dY[m, n]              fp32 [N], optional
//
// dY [M, N] and X [M, K] are row-major 16-bit (bf16 / fp16): the reduction runs over the STRIDED dimension of
// both operands, so neither MFMA operand can be read from LDS as stored.  Both come from the row-major LDS
// images by ds_read_b64_tr_b16, the transposed read of gp_attn_bwd.hip's read_transposed.
//
// Work item: one 256 (n) x 256 (k) output tile over one chunk of rows; 8 waves as 2 (n) x 4 (k), a wave owns
// 128 x 64 = 8 x 4 v_mfma_f32_16x16x32 tiles (128 fp32 accumulators per lane) with X^T as srcA and dY as srcB,
// so a lane holds 4 consecutive k of one n: 16-byte fp32 stores.
//
// Stage: 64 rows, dY[64 x 256] | X[64 x 256] = 2 x 32 KiB, two buffers (128 KiB, distinct __shared__ objects).
// Staging by LDS-DMA (buffer_load_dwordx4 ... lds), one wave-instruction = 1 KiB = two whole 512-byte row
// segments, lane-linear in LDS; the swizzle lives in the per-lane SOURCE address.  The descriptor is rebuilt
// per stage (64-bit base, so M < 2^31 rows never overflows a 32-bit offset) and its record count ends at the
// chunk's last row (<= M): rows past it arrive as zeros, no branch.  Each wave issues 8 loads per stage,
// unconditionally; stage s + 1 is issued right after the barrier that opens stage s and streams in under that
// stage's MFMAs, so the wait that opens stage s + 1 is vmcnt(0) with nothing else in flight.  (A deeper queue
// with a counted vmcnt(8) was tried first: the stage loop's trip count is a run-time value -- M is unbounded,
// the forward GEMM unrolls its K loop completely -- and hipcc's wait insertion turned the counted wait at the
// loop header into vmcnt(0), which left that scheme no lead at all.)
//
// Swizzle: a 512-byte LDS row is 16 pairs of 16-byte chunks (32 bytes = 16 columns); pair p of row r sits at
// pair p ^ (r & 7).  A transposed read's 16-lane group covers 4 rows x 32 bytes, the wave 16 consecutive rows
// x 32 bytes of one logical pair: rows r .. r + 7 land on the 8 distinct 32-byte slots of the 256-byte bank
// row, rows r + 8 .. r + 15 on the same 8 again -- 512 bytes over 64 banks x 4 bytes in the 2 passes the size
// needs, no conflict beyond them (derived; unswizzled, all 16 rows share one slot: 16 passes).
//
// Split over M: S chunks of `per` 64-row steps, S and per a function of (M, N, K) alone (wgrad_plan) -- never of
// the device -- so dW / db are bitwise reproducible from box to box.  S == 1 writes dW / db directly; otherwise
// the items write fp32 partials [S][N][K] (+ [S][N] column sums) to the workspace and wgrad_reduce_kernel adds
// them in chunk order.  No atomics.
//
// Bias gradient: the items of tile column k = 0 hold every dY stage already; each of their waves adds up 2 of
// the 8 dY fragments it has in registers for the MFMAs (a lane holds 8 rows of one column: 16 conversions + 16
// fp32 adds per k-step, in the shadow of 32 MFMAs), and the four lanes of a column meet once, in the epilogue.
// (An MFMA against a ones operand costs 12 more live registers -- the operand and two accumulator tiles -- and
// spilled; the sums cost 2.)
#include <stdint.h>

#include <type_traits>

#include "gp_api.h"
#include "gp_common.h"

namespace {

constexpr int kT = 256;                 // tile edge (n and k)
constexpr int kStep = 64;               // rows per stage
constexpr int kThreads = 512;
constexpr int kRowB = kT * 2;           // 512-byte LDS rows
constexpr int kImg = kStep * kRowB;     // one operand's stage: 32 KiB
constexpr int kTargetItems = 256;       // work items aimed at (one per CU of the largest part; a constant)
constexpr int kMinSteps = 4;            // no chunk shorter than 4 steps (256 rows): below that a partial's
                                        // 256 KiB write + read outweighs the 256 KiB of operands it covers

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef _Float16 f16x8w __attribute__((ext_vector_type(8)));
typedef int i32x4w __attribute__((ext_vector_type(4)));

__shared__ __attribute__((aligned(1024))) char w_buf0[2 * kImg];   // stages 0, 2, 4, ...: dY | X
__shared__ __attribute__((aligned(1024))) char w_buf1[2 * kImg];   // stages 1, 3, 5, ...
template <int B>
GP_DEV char* wbuf() {
  if constexpr (B == 0) return w_buf0;
  else return w_buf1;
}

struct WgradArgs {
  const uint16_t* dY;
  const uint16_t* X;
  float* out;        // S == 1: dW; else the workspace partials [S][N][K]
  float* bout;       // S == 1: db; else the workspace sums [S][N]; null: no bias gradient
  int64_t ldy, ldx, ldo;
  int64_t M;
  int N, K;
  int S, per;        // chunks, 64-row steps per chunk
};

template <int n>
GP_DEV void wait_vmcnt() {
  __builtin_amdgcn_s_waitcnt((n & 15) | ((n >> 4) << 14) | (0x7 << 4) | (0xf << 8));
}
GP_DEV void wg_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
  __builtin_amdgcn_sched_barrier(0);
}

template <bool kH>
GP_DEV f32x4 mfma(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  if constexpr (kH)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8w, a), __builtin_bit_cast(f16x8w, b), c, 0, 0,
                                                  0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// One fragment of a k-step's 32 rows: lane (l16, g4) gets column (fragment base + l16), rows 4 g4 .. + 3 and
// 16 + 4 g4 .. + 3 of the k-step -- the same row order for both operands, so the MFMA contracts matching rows.
GP_DEV bf16x8 read_tr(const char* p) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 16 * kRowB));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <bool kH, bool kBias>
__global__ __launch_bounds__(kThreads, 1) void wgrad_kernel(const WgradArgs g) {
  const int tiles_k = g.K / kT;
  const int tiles = (g.N / kT) * tiles_k;
  // chunk-major item order: the items running together share one chunk's rows of dY and X in L2
  const int s = (int)blockIdx.x / tiles, t = (int)blockIdx.x % tiles;
  const int tn = t / tiles_k, tk = t % tiles_k;
  const int64_t row0 = (int64_t)s * g.per * kStep;
  const int64_t row_end = g.M - row0 < (int64_t)g.per * kStep ? g.M : row0 + (int64_t)g.per * kStep;
  const int nst = (int)((row_end - row0 + kStep - 1) / kStep);   // >= 1 (wgrad_plan leaves no empty chunk)

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int wn = w >> 2, wk = w & 3;
  const int l16 = lane & 15, g4 = lane >> 4;

  // LDS-DMA: instruction j of wave w covers stage rows 16 j + 2 w, + 1; lane l writes row + l / 32, physical
  // chunk l % 32, which holds logical chunk (l % 32) ^ ((row & 7) << 1).  row & 7 does not depend on j: one
  // per-lane offset per operand, the 16 j rows in the scalar offset.
  int voff[2];
  {
    const int r = 2 * w + (lane >> 5);
    const int c = (lane & 31) ^ ((r & 7) << 1);
    voff[0] = (int)((int64_t)r * g.ldy * 2) + c * 16;
    voff[1] = (int)((int64_t)r * g.ldx * 2) + c * 16;
  }
  const int soff[2] = {(int)(16 * g.ldy * 2), (int)(16 * g.ldx * 2)};
  const uint16_t* ybase = g.dY + (int64_t)tn * kT;
  const uint16_t* xbase = g.X + (int64_t)tk * kT;
  // stage st of the chunk into buffer B.  Rows at or past row_end (the chunk's end, <= M) lie beyond the record
  // count and arrive as zeros: the stage after the chunk's last one, issued unconditionally, loads nothing.
  auto issue = [&](auto bc, int st) {
    constexpr int B = decltype(bc)::value;
    const int64_t r0 = row0 + (int64_t)st * kStep;
    int64_t rem = row_end - r0;
    rem = rem < 0 ? 0 : (rem > kStep ? kStep : rem);
    const int64_t r0c = rem > 0 ? r0 : row0;   // (no pointer past the operand when nothing is read)
    const int ny = rem > 0 ? (int)((rem - 1) * g.ldy * 2 + kRowB) : 0;
    const int nx = rem > 0 ? (int)((rem - 1) * g.ldx * 2 + kRowB) : 0;
    const __amdgpu_buffer_rsrc_t ry =
        __builtin_amdgcn_make_buffer_rsrc((void*)(ybase + r0c * g.ldy), (short)0, ny, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc((void*)(xbase + r0c * g.ldx), (short)0, nx, 0x00020000);
    char* dst = wbuf<B>() + w * 1024;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ry, (__attribute__((address_space(3))) void*)(dst + j * 16 * kRowB), 16,
                                               voff[0], j * soff[0], 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(dst + kImg + j * 16 * kRowB),
                                               16, voff[1], j * soff[1], 0, 0);
  };

  // transposed fragment reads: lane (l16, g4) addresses k-step row 4 g4 + l16 / 4, bytes 8 (l16 % 4) .. + 7 of the
  // fragment's 32-byte pair; pair index p (wave n / k offset + fragment f) sits at p ^ (row & 7).  The wave's
  // pair offset is a multiple of the fragment count, so (p0 + f) ^ x = (p0 ^ x) ^ f, and the pair index fills
  // address bits 5-8, which are zero in the row / byte part: fragment f's address is fragment 0's ^ (f << 5).
  const int rowl = 4 * g4 + (l16 >> 2), rx7 = rowl & 7;
  const int lbase = rowl * kRowB + (l16 & 3) * 8;
  const int offn0 = lbase + (((wn * 8) ^ rx7) << 5);
  const int offk0 = lbase + (((wk * 4) ^ rx7) << 5);

  f32x4 acc[8][4];
#pragma unroll
  for (int nf = 0; nf < 8; ++nf)
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) acc[nf][kf] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sb[2] = {0.f, 0.f};
  const bool bias_item = kBias && tk == 0;
  typedef uint32_t u32x4w __attribute__((ext_vector_type(4)));

  auto compute = [&](auto bc) {
    constexpr int B = decltype(bc)::value;
    const char* buf = wbuf<B>();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fy[8], fx[4];
      // opaque per k-step: the 12 fragment addresses are then formed where they are used (one v_xor each)
      // instead of being hoisted out of the stage loop into 12 more live registers
      int on = offn0, ok = offk0;
      asm volatile("" : "+v"(on), "+v"(ok));
#pragma unroll
      for (int f = 0; f < 8; ++f) fy[f] = read_tr(buf + ks * 32 * kRowB + (on ^ (f << 5)));
#pragma unroll
      for (int f = 0; f < 4; ++f) fx[f] = read_tr(buf + kImg + ks * 32 * kRowB + (ok ^ (f << 5)));
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int nf = 0; nf < 8; ++nf)
#pragma unroll
        for (int kf = 0; kf < 4; ++kf) acc[nf][kf] = mfma<kH>(fx[kf], fy[nf], acc[nf][kf]);
      __builtin_amdgcn_s_setprio(0);
      if constexpr (kBias) {
        if (bias_item) {   // (wave-uniform) this wave's share: dY fragments 2 wk, 2 wk + 1, picked by selects on
                           // the wave-uniform wk (register arrays cannot be indexed by it; no branch per fragment)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            u32x4w u = __builtin_bit_cast(u32x4w, fy[e]);
#pragma unroll
            for (int p = 1; p < 4; ++p) {
              const u32x4w v = __builtin_bit_cast(u32x4w, fy[2 * p + e]);
#pragma unroll
              for (int d = 0; d < 4; ++d) u[d] = wk == p ? v[d] : u[d];
            }
#pragma unroll
            for (int d = 0; d < 4; ++d) sb[e] = (sb[e] + e2f<kH>(u[d])) + e2f_hi<kH>(u[d]);
          }
        }
      }
      // (the next k-step's 12 fragments are not read ahead of this one's MFMAs: 48 more live registers spill;
      // the SIMD's other wave covers the reads)
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // stage st in buffer B: its loads (issued one stage earlier) landed, for this wave and -- past the barrier -- for
  // every wave; the same barrier says every wave is done with stage st - 1, so the other buffer takes stage
  // st + 1, which streams in under this stage's 64 MFMAs.  One barrier per stage.
  auto stage = [&](auto bc, auto bnext, int st) {
    wait_vmcnt<0>();
    wg_barrier();
    issue(bnext, st + 1);
    compute(bc);
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  issue(I0(), 0);
  for (int st = 0; st < nst; st += 2) {
    stage(I0(), I1(), st);
    stage(I1(), I0(), st + 1);   // (past an odd chunk's end: a stage of zeros)
  }
  wait_vmcnt<0>();   // no LDS-DMA in flight at exit

  // Epilogue.  Lane (l16, g4) holds, for n-frag nf and k-frag kf, dW[nb + 16 nf + l16][kb + 16 kf + 4 g4 .. + 3].
  // Whole 128-byte lines: for a k-frag pair one DPP row_ror:8 per dword hands rows 8-15's first half-line to
  // lanes 0-7 and rows 0-7's second half-line to lanes 8-15 of every 16-lane row, so each 16-byte store writes
  // 8 rows x 32 consecutive floats (the scheme of gp_gemm_impl.h's store_mfrag).
  float* obase = g.out + (g.S > 1 ? (int64_t)s * g.N * g.ldo : 0) + (int64_t)(tn * kT + wn * 128) * g.ldo + tk * kT +
                 wk * 64;
  const uint64_t op = reinterpret_cast<uint64_t>(obase);
  const uint64_t opu = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(op >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)op);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<void*>(opu), (short)0, __builtin_amdgcn_readfirstlane((int)((127 * g.ldo + 64) * 4)), 0x00020000);
  const bool lo8 = l16 < 8;
  const int o_lane = (int)(((l16 & 7) * g.ldo + (lo8 ? 0 : 16) + 4 * g4) * 4);
  const int o_nf = (int)(16 * g.ldo * 4), o_hi = (int)(8 * g.ldo * 4);
#pragma unroll
  for (int nf = 0; nf < 8; ++nf)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const i32x4w a0 = __builtin_bit_cast(i32x4w, acc[nf][2 * p]), a1 = __builtin_bit_cast(i32x4w, acc[nf][2 * p + 1]);
      i32x4w V[2];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int r0 = __builtin_amdgcn_update_dpp(0, a0[d], 0x128, 0xf, 0xf, false);   // row_ror:8
        const int r1 = __builtin_amdgcn_update_dpp(0, a1[d], 0x128, 0xf, 0xf, false);
        V[0][d] = lo8 ? a0[d] : r1;   // rows 0-7
        V[1][d] = lo8 ? r0 : a1[d];   // rows 8-15
      }
      // (two wait states after every store: the store-data hazard of DESIGN §3.4)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        __builtin_amdgcn_raw_buffer_store_b128(V[hh], ro, o_lane, nf * o_nf + hh * o_hi + p * 128, 0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 1");
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  if constexpr (kBias) {
    // lane (l16, g4) holds the sum of column l16 over the rows of its g4: the four meet, g4 == 0 writes
    if (bias_item) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        sb[e] += __shfl_xor(sb[e], 16, 64);
        sb[e] += __shfl_xor(sb[e], 32, 64);
      }
      if (g4 == 0) {
        float* bo = g.bout + (g.S > 1 ? (int64_t)s * g.N : 0) + tn * kT + wn * 128 + wk * 32 + l16;
        bo[0] = sb[0];
        bo[16] = sb[1];
      }
    }
  }
}

// dW = the S partials added in chunk order (one thread per 4 columns of a row); the threads past them do db.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* ws, float* dW, int64_t ldw, float* db, int N,
                                                           int K, int S) {
  const int64_t nk = (int64_t)N * K;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nk / 4) {
    const int64_t e = i * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(ws + e);
    for (int s = 1; s < S; ++s) v += *reinterpret_cast<const f32x4*>(ws + s * nk + e);
    *reinterpret_cast<f32x4*>(dW + (e / K) * ldw + e % K) = v;
  } else if (db != nullptr && i - nk / 4 < N) {
    const float* p = ws + (int64_t)S * nk + (i - nk / 4);
    float v = p[0];
    for (int s = 1; s < S; ++s) v += p[(int64_t)s * N];
    db[i - nk / 4] = v;
  }
}

// S chunks of `per` 64-row steps: about kTargetItems items, no chunk shorter than kMinSteps steps, none empty.
// A function of the shape alone.
void wgrad_plan(int64_t M, int64_t N, int64_t K, int& S, int& per) {
  const int64_t tiles = (N / kT) * (K / kT);
  const int64_t steps = (M + kStep - 1) / kStep;
  int64_t want = kTargetItems / tiles;
  const int64_t most = steps / kMinSteps;
  if (want > most) want = most;
  if (want < 1) want = 1;
  const int64_t p = (steps + want - 1) / want;
  per = (int)p;
  S = (int)((steps + p - 1) / p);
}

bool wgrad_shape_ok(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && M < (int64_t)0x7fffffff && N > 0 && K > 0 && N % kT == 0 && K % kT == 0 &&
         (N / kT) * (K / kT) <= 65536;
}

}  // namespace

extern "C" int64_t gp_linear_wgrad_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (!wgrad_shape_ok(M, N, K)) return 0;
  int S, per;
  wgrad_plan(M, N, K, S, per);
  return S > 1 ? (int64_t)S * (N * K + N) * (int64_t)sizeof(float) : 0;
}

extern "C" int gp_linear_wgrad(const uint16_t* dY, int64_t ldy, const uint16_t* X, int64_t ldx, float* dW, int64_t ldw,
                               float* db, int64_t M, int64_t N, int64_t K, void* ws, int64_t ws_bytes, int fmt,
                               void* stream) {
  const char* who = "gp_linear_wgrad";
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16, "%s: bad fmt %d (GP_FMT_BF16 or GP_FMT_F16)", who, fmt);
  GP_REQUIRE(dY && X && dW, "%s: null pointer", who);
  GP_REQUIRE(M >= 1 && M < (int64_t)0x7fffffff, "%s: M=%lld outside [1, 2^31)", who, (long long)M);
  GP_REQUIRE(N > 0 && N % kT == 0, "%s: N=%lld must be a positive multiple of %d", who, (long long)N, kT);
  GP_REQUIRE(K > 0 && K % kT == 0, "%s: K=%lld must be a positive multiple of %d", who, (long long)K, kT);
  GP_REQUIRE(wgrad_shape_ok(M, N, K), "%s: too many output tiles (N=%lld, K=%lld)", who, (long long)N, (long long)K);
  GP_REQUIRE(ldy >= N && ldx >= K && ldw >= K && ldy % 8 == 0 && ldx % 8 == 0 && ldw % 4 == 0,
             "%s: bad leading dimensions", who);
  GP_REQUIRE(gp_aligned(dY, 16) && gp_aligned(X, 16) && gp_aligned(dW, 16) && (db == nullptr || gp_aligned(db, 16)),
             "%s: misaligned operand", who);
  GP_REQUIRE((int64_t)kStep * ldy * 2 < 0x7fffffff && (int64_t)kStep * ldx * 2 < 0x7fffffff &&
                 (int64_t)128 * ldw * 4 < 0x7fffffff,
             "%s: leading dimension too large for 32-bit tile offsets", who);
  int S, per;
  wgrad_plan(M, N, K, S, per);
  const int64_t need = gp_linear_wgrad_workspace_bytes(M, N, K);
  if (S > 1) {
    GP_REQUIRE(ws && ws_bytes >= need, "%s: workspace too small (%lld bytes, need %lld)", who,
               (long long)(ws ? ws_bytes : 0), (long long)need);
    GP_REQUIRE(gp_aligned(ws, 16), "%s: misaligned workspace", who);
  }
  WgradArgs a;
  a.dY = dY;
  a.X = X;
  a.ldy = ldy;
  a.ldx = ldx;
  a.M = M;
  a.N = (int)N;
  a.K = (int)K;
  a.S = S;
  a.per = per;
  if (S > 1) {
    a.out = static_cast<float*>(ws);
    a.bout = db != nullptr ? a.out + (int64_t)S * N * K : nullptr;
    a.ldo = K;
  } else {
    a.out = dW;
    a.bout = db;
    a.ldo = ldw;
  }
  const hipStream_t st = gp_stream(stream);
  const dim3 grid((unsigned)((N / kT) * (K / kT) * S)), block(kThreads);
  const bool kh = fmt == GP_FMT_F16;
  if (db != nullptr) {
    if (kh) wgrad_kernel<true, true><<<grid, block, 0, st>>>(a);
    else wgrad_kernel<false, true><<<grid, block, 0, st>>>(a);
  } else {
    if (kh) wgrad_kernel<true, false><<<grid, block, 0, st>>>(a);
    else wgrad_kernel<false, false><<<grid, block, 0, st>>>(a);
  }
  if (S > 1) {
    const int64_t thr = N * K / 4 + (db != nullptr ? N : 0);
    wgrad_reduce_kernel<<<(unsigned)((thr + 255) / 256), 256, 0, st>>>(a.out, dW, ldw, db, (int)N, (int)K, S);
  }
  return gp_check_launch(who);
}
