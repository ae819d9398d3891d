// Data gradient of nn.Linear on gfx950 MFMAs (gp_linear_dgrad): the backward of the QKV / out-proj / fc1 / fc2
// projections of the training path for their input (multihead_attention.py:43-48, feedforward_network.py:131-142).
//
//   dX[m, k] = sum_{n < N} dY[m, n] W[n, k]      16-bit [M, ldx], rounded once from the fp32 sum
//
// dY [M, N] is contiguous along the reduction, W [N, K] is contracted over its ROWS: the forward GEMM's operand
// layout (both contiguous along the reduction) fits only dY.  W comes from its row-major LDS image by
// ds_read_b64_tr_b16, as gp_gemm_wgrad.hip reads its X; no transposed copy of W is ever made.
//
// Work item: one 256 (m) x 256 (k) output tile over the whole reduction; 8 waves as 2 (m) x 4 (k), a wave owns
// 128 x 64 = 8 x 4 v_mfma_f32_16x16x32 tiles (128 fp32 accumulators per lane) with W^T as srcA and dY as srcB, so
// a lane holds 4 consecutive k of one m.  One item per workgroup, row block major: the K / 256 items of one row
// block are neighbours in the grid and share its dY rows in L2; W (at most 9.4 MB) stays in L2 for every row block.
//
// Stage: 64 of n, dY[256 m x 64 n] | W[64 n x 256 k] = 2 x 32 KiB, two buffers (128 KiB, distinct __shared__
// objects).  Staging by LDS-DMA (buffer_load_dwordx4 ... lds), one wave-instruction = 1 KiB, lane-linear in LDS;
// swizzles and the row permutation below live in the per-lane SOURCE address.  Descriptors are rebuilt per stage
// from 64-bit bases: no 32-bit offset spans more than one stage of the tile.  The dY descriptor ends at the row
// block's last row (<= M): rows past it arrive as zeros, no branch.  Each wave issues 8 loads per stage; stage
// s + 1 is issued right after the barrier that opens stage s and streams in under that stage's 64 MFMAs, so the
// wait that opens s + 1 is vmcnt(0) with nothing else in flight (gp_gemm_wgrad.hip's scheme: the trip count N / 64
// is a run-time value, and a counted vmcnt at such a loop's header is turned into vmcnt(0) by hipcc).
//
// W image: 512-byte rows, wgrad's pair swizzle: 32-byte pair p of LDS row r sits at pair p ^ (r & 7).  The rows of a
// 32-row k-step are stored PERMUTED: LDS row 16 h + 4 g + j holds reduction index 8 g + 4 h + j.  A transposed read
// hands lane group g4 LDS rows 4 g4 .. + 3 and 16 + 4 g4 .. + 3, which are then the 8 CONSECUTIVE indices 8 g4 .. + 7:
// the matching dY fragment is one 16-byte ds_read_b128 of dY[m][8 g4 .. + 7] instead of two 8-byte reads.  (The
// permutation costs nothing: the DMA's source row is a per-lane / per-instruction offset either way.)
//
// dY image: 128-byte rows = 8 chunks of 16 bytes; chunk c of row r sits at chunk c ^ ((r >> 1) & 7).  A fragment
// read takes, for each lane group g4, chunk 4 ks + g4 of 16 consecutive rows: two rows share a 256-byte bank row,
// r & 1 picks its half, (r >> 1) & 7 spreads the 8 row pairs over the half's 8 chunk slots -- the 16 lanes of a
// group hit 16 distinct 16-byte slots, the wave's 1 KiB goes through 64 banks x 4 bytes in the 4 passes its size
// needs (derived, not measured; unswizzled, 8 rows share each slot: 8 times that).
//
// Epilogue: fp32 -> fmt by v_cvt_pk, then lane groups g4 and g4 ^ 1 trade one k-fragment of each pair, so a lane
// holds 8 consecutive k of its row: one 16-byte store, 64 contiguous bytes per row per wave-instruction.  The
// wave's dX descriptor ends at the row block's last row: rows at or past M are dropped by the bounds check.
#include <stdint.h>

#include <type_traits>

#include "gp_api.h"
#include "gp_common.h"

namespace {

constexpr int kT = 256;                 // tile edge (m and k)
constexpr int kStep = 64;               // reduction indices per stage
constexpr int kThreads = 512;
constexpr int kRowW = kT * 2;           // W image: 512-byte LDS rows
constexpr int kRowY = kStep * 2;        // dY image: 128-byte LDS rows
constexpr int kImg = kT * kStep * 2;    // one operand's stage: 32 KiB

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) void lds_void;
typedef _Float16 f16x8w __attribute__((ext_vector_type(8)));
typedef int i32x4w __attribute__((ext_vector_type(4)));

__shared__ __attribute__((aligned(1024))) char d_buf0[2 * kImg];   // stages 0, 2, 4, ...: dY | W
__shared__ __attribute__((aligned(1024))) char d_buf1[2 * kImg];   // stages 1, 3, 5, ...
template <int B>
GP_DEV char* dbuf() {
  if constexpr (B == 0) return d_buf0;
  else return d_buf1;
}

struct DgradArgs {
  const uint16_t* dY;
  const uint16_t* W;
  uint16_t* dX;
  int64_t ldy, ldw, ldx;
  int64_t M;
  int N, K;
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

// One W fragment of a k-step: lane (l16, g4) gets column (fragment base + l16) of LDS rows 4 g4 .. + 3 and
// 16 + 4 g4 .. + 3 of the k-step, which hold the reduction indices 8 g4 .. + 7 in order.
GP_DEV bf16x8 read_tr(const char* p) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 16 * kRowW));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <bool kH>
__global__ __launch_bounds__(kThreads, 1) void dgrad_kernel(const DgradArgs g) {
  const int tiles_k = g.K / kT;
  // row block major: the tiles_k items of one row block run together
  const int64_t tm = (int64_t)(blockIdx.x / (unsigned)tiles_k);
  const int tk = (int)(blockIdx.x % (unsigned)tiles_k);
  const int64_t m0 = tm * kT;
  const int rows = g.M - m0 < kT ? (int)(g.M - m0) : kT;   // 1 .. 256 rows of dY / dX in this block
  const int nst = g.N / kStep;   // even, as the two-buffer loop below needs: the host requires N % 256 == 0

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int wm = w >> 2, wk = w & 3;
  const int l16 = lane & 15, g4 = lane >> 4;

  // LDS-DMA.  dY: instruction j of wave w covers block rows 64 j + 8 w .. + 7; lane l writes row + l / 8, physical
  // chunk l % 8, which holds logical chunk (l % 8) ^ ((row >> 1) & 7) -- bits 1-3 of the row do not depend on j.
  // W: instruction j covers LDS rows 16 j + 2 w, + 1 of the stage; lane l writes row + l / 32, physical chunk
  // l % 32, which holds logical chunk (l % 32) ^ ((row & 7) << 1); LDS row 32 ks + 16 h + 4 g + jj (j = 2 ks + h,
  // 2 w + l / 32 = 4 g + jj) is fed from reduction index 32 ks + 8 g + 4 h + jj of the stage.
  int voff_y, voff_w;
  {
    const int ry = 8 * w + (lane >> 3);
    voff_y = (int)((int64_t)ry * g.ldy * 2) + (((lane & 7) ^ ((ry >> 1) & 7)) << 4);
    const int rw = 2 * w + (lane >> 5);
    voff_w = (int)((int64_t)(8 * (rw >> 2) + (rw & 3)) * g.ldw * 2) + (((lane & 31) ^ ((rw & 7) << 1)) << 4);
  }
  const int soff_y = (int)(64 * g.ldy * 2);   // per j: 64 block rows
  const int soff_w4 = (int)(4 * g.ldw * 2), soff_w32 = (int)(32 * g.ldw * 2);
  const uint16_t* ybase = g.dY + m0 * g.ldy;
  const uint16_t* wbase = g.W + (int64_t)tk * kT;
  const int ny = (int)((int64_t)(rows - 1) * g.ldy * 2) + kRowY;   // the block's rows, this stage's 64 columns
  const int nw = (int)((int64_t)(kStep - 1) * g.ldw * 2) + kRowW;  // the stage's 64 rows, the tile's 256 columns
  // stage st into buffer B; the stage after the last one, issued unconditionally, has empty descriptors
  auto issue = [&](auto bc, int st) {
    constexpr int B = decltype(bc)::value;
    const bool live = st < nst;
    const int stc = live ? st : 0;   // (no pointer past the operands when nothing is read)
    const __amdgpu_buffer_rsrc_t ry =
        __builtin_amdgcn_make_buffer_rsrc((void*)(ybase + stc * kStep), (short)0, live ? ny : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(wbase + (int64_t)stc * kStep * g.ldw),
                                                                        (short)0, live ? nw : 0, 0x00020000);
    char* dst = dbuf<B>() + w * 1024;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ry, (lds_void*)(dst + j * 64 * kRowY), 16, voff_y, j * soff_y, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void*)(dst + kImg + j * 16 * kRowW), 16, voff_w,
                                               (j >> 1) * soff_w32 + (j & 1) * soff_w4, 0, 0);
  };

  // W fragments (transposed reads): lane (l16, g4) addresses k-step LDS row 4 g4 + l16 / 4, bytes 8 (l16 % 4) .. + 7
  // of the fragment's 32-byte pair; pair p (wave offset 4 wk + fragment f) sits at p ^ (row & 7), and since the wave
  // offset is a multiple of the fragment count, fragment f's address is fragment 0's ^ (f << 5).
  // dY fragments (plain reads): lane (l16, g4) reads row 128 wm + 16 f + l16, logical chunk 4 ks + g4, physical
  // chunk that ^ ((row >> 1) & 7) = that ^ (l16 >> 1): fragment f's address is fragment 0's + f * 16 rows.
  const int rowl = 4 * g4 + (l16 >> 2);
  const int offw0 = rowl * kRowW + (l16 & 3) * 8 + (((wk * 4) ^ (rowl & 7)) << 5);
  const int offy0 = (wm * 128 + l16) * kRowY;
  const int cy[2] = {(g4 ^ (l16 >> 1)) << 4, ((4 + g4) ^ (l16 >> 1)) << 4};

  f32x4 acc[8][4];
#pragma unroll
  for (int mf = 0; mf < 8; ++mf)
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) acc[mf][kf] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](auto bc) {
    constexpr int B = decltype(bc)::value;
    const char* buf = dbuf<B>();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fy[8], fw[4];
      // opaque per k-step: the fragment addresses are formed where they are used instead of being hoisted out of
      // the stage loop into more live registers
      int oy = offy0 + cy[ks], ow = offw0;
      asm volatile("" : "+v"(oy), "+v"(ow));
#pragma unroll
      for (int f = 0; f < 8; ++f) fy[f] = *reinterpret_cast<const bf16x8*>(buf + oy + f * 16 * kRowY);
#pragma unroll
      for (int f = 0; f < 4; ++f) fw[f] = read_tr(buf + kImg + ks * 32 * kRowW + (ow ^ (f << 5)));
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mf = 0; mf < 8; ++mf)
#pragma unroll
        for (int kf = 0; kf < 4; ++kf) acc[mf][kf] = mfma<kH>(fw[kf], fy[mf], acc[mf][kf]);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // stage st in buffer B: its loads (issued one stage earlier) landed, for this wave and -- past the barrier -- for
  // every wave; the same barrier says every wave is done with stage st - 1, so the other buffer takes stage st + 1.
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
    stage(I1(), I0(), st + 1);
  }
  wait_vmcnt<0>();   // no LDS-DMA in flight at exit (the last issue had empty descriptors)

  // Epilogue.  Lane (l16, g4) holds, for m-frag mf and k-frag kf, dX[mb + 16 mf + l16][kb + 16 kf + 4 g4 .. + 3].
  // Per k-frag pair, lane groups g4 and g4 ^ 1 trade: the even group keeps fragment 2p and gets its neighbour's
  // (k 4 g4 .. + 7 of the pair's 32), the odd group keeps 2p + 1 and gets its neighbour's (k 16 + 4 (g4 - 1) .. + 7).
  const int wrows = rows - wm * 128;   // rows of this wave's half of the block (<= 0: none)
  const int64_t mrow = wrows > 0 ? m0 + wm * 128 : m0;
  uint16_t* obase = g.dX + mrow * g.ldx + tk * kT + wk * 64;
  const uint64_t op = reinterpret_cast<uint64_t>(obase);
  const uint64_t opu = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(op >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)op);
  const int nrec = wrows > 0 ? (int)((int64_t)((wrows < 128 ? wrows : 128) - 1) * g.ldx * 2) + 64 * 2 : 0;
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<void*>(opu), (short)0, __builtin_amdgcn_readfirstlane(nrec), 0x00020000);
  const bool even = (g4 & 1) == 0;
  const int o_lane = (int)((int64_t)l16 * g.ldx * 2) + (even ? 4 * g4 : 16 + 4 * (g4 - 1)) * 2;
  const int o_mf = (int)(16 * g.ldx * 2);
#pragma unroll
  for (int mf = 0; mf < 8; ++mf)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const f32x4 a0 = acc[mf][2 * p], a1 = acc[mf][2 * p + 1];
      const int c0[2] = {(int)pack2e<kH>(a0[0], a0[1]), (int)pack2e<kH>(a0[2], a0[3])};
      const int c1[2] = {(int)pack2e<kH>(a1[0], a1[1]), (int)pack2e<kH>(a1[2], a1[3])};
      i32x4w V;
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const int t = __shfl_xor(even ? c1[d] : c0[d], 16, 64);
        V[d] = even ? c0[d] : t;
        V[2 + d] = even ? t : c1[d];
      }
      // (two wait states after every store: the store-data hazard of DESIGN §3.4)
      __builtin_amdgcn_raw_buffer_store_b128(V, ro, o_lane, mf * o_mf + p * 64, 0);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_nop 1");
      __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace

extern "C" int gp_linear_dgrad(const uint16_t* dY, int64_t ldy, const uint16_t* W, int64_t ldw, uint16_t* dX,
                               int64_t ldx, int64_t M, int64_t N, int64_t K, int fmt, void* stream) {
  const char* who = "gp_linear_dgrad";
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16, "%s: bad fmt %d (GP_FMT_BF16 or GP_FMT_F16)", who, fmt);
  GP_REQUIRE(dY && W && dX, "%s: null pointer", who);
  GP_REQUIRE(M >= 1 && M < (int64_t)0x7fffffff, "%s: M=%lld outside [1, 2^31)", who, (long long)M);
  GP_REQUIRE(N > 0 && N % kT == 0, "%s: N=%lld must be a positive multiple of %d", who, (long long)N, kT);
  GP_REQUIRE(K > 0 && K % kT == 0, "%s: K=%lld must be a positive multiple of %d", who, (long long)K, kT);
  GP_REQUIRE(N < (int64_t)0x7fffffff && K < (int64_t)0x7fffffff && ((M + kT - 1) / kT) * (K / kT) < (int64_t)0x7fffffff,
             "%s: too many output tiles (M=%lld, K=%lld)", who, (long long)M, (long long)K);
  GP_REQUIRE(ldy >= N && ldw >= K && ldx >= K && ldy % 8 == 0 && ldw % 8 == 0 && ldx % 8 == 0,
             "%s: bad leading dimensions (at least the row length, multiples of 8)", who);
  GP_REQUIRE(gp_aligned(dY, 16) && gp_aligned(W, 16) && gp_aligned(dX, 16), "%s: misaligned operand", who);
  GP_REQUIRE((int64_t)kT * ldy * 2 < 0x7fffffff && (int64_t)kStep * ldw * 2 < 0x7fffffff &&
                 (int64_t)kT * ldx * 2 < 0x7fffffff,
             "%s: leading dimension too large for 32-bit tile offsets", who);
  DgradArgs a;
  a.dY = dY;
  a.W = W;
  a.dX = dX;
  a.ldy = ldy;
  a.ldw = ldw;
  a.ldx = ldx;
  a.M = M;
  a.N = (int)N;
  a.K = (int)K;
  const dim3 grid((unsigned)(((M + kT - 1) / kT) * (K / kT))), block(kThreads);
  const hipStream_t st = gp_stream(stream);
  if (fmt == GP_FMT_F16) dgrad_kernel<true><<<grid, block, 0, st>>>(a);
  else dgrad_kernel<false><<<grid, block, 0, st>>>(a);
  return gp_check_launch(who);
}
