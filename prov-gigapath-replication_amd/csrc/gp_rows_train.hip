// Row kernels of the training path at the model width (gp_resid_drop_ln_fwd / gp_resid_drop_ln_bwd /
// gp_dropout_keep_mask): residual add with dropout and drop-path, and the LayerNorm that follows it, forward and
// backward.  A translation unit of its own, so that the code object of the inference row kernels (gp_norm.hip) is
// not touched by it.
//
// Forward, per row (fp32 arithmetic):
//   r = x + f y,  f[col] = keep(seed, row cols + col) ? s[row / rows_per_scale] / (1 - p) : 0      (fp32, stored)
//   a = round_fmt(LayerNorm(r) ln_w + ln_b)                                                          (16-bit)
// as (A) both lines, (B) the first line only, (C) the second line only, on an fp32 or a 16-bit input.  One device
// routine does the add (row_add) and one the LayerNorm (row_ln_stats + row_ln_store), with every multiply-add
// spelled as fmaf and contraction off, so that (A) gives the bits of (B) followed by (C) on its r.
//
// Dropout mask.  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; multipliers
// 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85, ten rounds, the key bumped between rounds):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (q & 0xffffffff, q >> 32, 0, 0),  q = (row cols + col) >> 2        (cols % 4 == 0)
//   word j of the four output words serves element index 4 q + j
//   keep    = word >= T,  T = floor(p 2^32) computed on the host in double          (P[keep] = 1 - T / 2^32)
// T == 0 (p == 0) keeps everything and runs no generator.  The mask depends on (seed, element index, p) alone --
// not on the grid, the block or the wave -- and is never stored: the backward regenerates it with the same routine
// (drop_keep4), and gp_dropout_keep_mask writes it out as bytes with that routine.
//
// Layout: a 64-lane wave per row, four waves per block, rows grid-stride by wave; lane l owns the columns
// k 256 + 4 l + {0..3}, k < cols / 256 (one Philox call per lane and k).  The next row's loads are issued
// unconditionally before the current row's arithmetic (past the end a wave re-reads the last row and drops it), so a
// row is in registers before anything of it is written: r may be x, and dx may be dr_in.
// Backward parameter sums (kParam): every lane sums da xhat (in double) and da over the rows of its wave; the four
// waves are added in wave order through LDS and the block writes one [2][cols] fp32 partial; rows_bwd_reduce_kernel
// adds the partials in block order, in double, and rounds once.  No atomics, and the grid is a function of (rows, cols) alone, so dln_w / dln_b are the
// same bits on every run and every device.
#include <math.h>
#include <stdlib.h>

#include <type_traits>

#include "gp_api.h"
#include "gp_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kRowsFwdMaxBlocks = 2048;
constexpr int kRowsBwdMaxBlocks = 1024;

// Dropout and drop-path of one call.  s: one fp32 factor per rps rows or NULL (= 1); thr: the keep threshold T;
// inv: 1 / (1 - p) rounded to fp32 on the host; k0 / k1: the Philox key.
struct RowDrop {
  const float* s;
  uint32_t rps;
  uint32_t thr;
  float inv;
  uint32_t k0, k1;
};

GP_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                          uint32_t (&out)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// keep[j] for the element indices 4 q + j
GP_DEV void drop_keep4(uint32_t k0, uint32_t k1, uint32_t thr, uint64_t q, bool (&keep)[4]) {
  uint32_t w[4];
  philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), 0u, 0u, k0, k1, w);
#pragma unroll
  for (int j = 0; j < 4; ++j) keep[j] = w[j] >= thr;
}

// f[i] of a row: the row's scale m = s[row / rps] * inv where kept, 0 where dropped
template <int EPL>
GP_DEV void row_factors(const RowDrop& d, uint32_t row, int lane, float (&f)[EPL]) {
  float m = d.inv;
  if (d.s) m = d.s[row / d.rps] * d.inv;
  if (d.thr == 0) {
#pragma unroll
    for (int i = 0; i < EPL; ++i) f[i] = m;
    return;
  }
  const uint64_t q0 = (uint64_t)row * (uint64_t)(EPL * 16) + (uint64_t)lane;     // (row cols + 4 lane) / 4
#pragma unroll
  for (int k = 0; k < EPL / 4; ++k) {
    bool keep[4];
    drop_keep4(d.k0, d.k1, d.thr, q0 + (uint64_t)(k * 64), keep);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[4 * k + j] = keep[j] ? m : 0.f;
  }
}

// v += f y
template <int EPL>
GP_DEV void row_add(float (&v)[EPL], const float (&y)[EPL], const float (&f)[EPL]) {
#pragma unroll
  for (int i = 0; i < EPL; ++i) v[i] = fmaf(f[i], y[i], v[i]);
}

// torch's LayerNorm statistics: biased variance, two passes, fp32
template <int EPL>
GP_DEV void row_ln_stats(const float (&v)[EPL], float eps, float& mean, float& rstd) {
  constexpr float kC = (float)(64 * EPL);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < EPL; ++i) s += v[i];
  mean = wave_sum(s) / kC;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < EPL; ++i) {
    const float d = v[i] - mean;
    q = fmaf(d, d, q);
  }
  // correctly rounded 1 / sqrt (once per row): dx is compared at fp32 level, v_rsq_f32's last-bit error is a row scale
  rstd = 1.0f / sqrtf(wave_sum(q) / kC + eps);
}

template <int EPL, bool kH>
GP_DEV void row_ln_store(const float (&v)[EPL], float mean, float rstd, const float (&w)[EPL], const float (&b)[EPL],
                         uint16_t* arow, int lane) {
  float o[EPL];
#pragma unroll
  for (int i = 0; i < EPL; ++i) o[i] = fmaf((v[i] - mean) * rstd, w[i], b[i]);
  st_x4_e<kH, EPL>(arow, lane, o);
}

// A row in its memory form: fp32 (float4 per chunk) or 16-bit (uint2 per chunk), lane mapping "x4"
template <int EPL, bool k16>
struct RowRegs {
  static constexpr int NK = EPL / 4;
  typename std::conditional<k16, uint2, float4>::type u[NK];
  GP_DEV void load(const void* base, size_t row_off, int lane) {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      if constexpr (k16)
        u[k] = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(base) + row_off + k * 256 + 4 * lane);
      else
        u[k] = *reinterpret_cast<const float4*>(static_cast<const float*>(base) + row_off + k * 256 + 4 * lane);
    }
  }
  template <bool kH>
  GP_DEV void unpack(float (&v)[EPL]) const {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      if constexpr (k16) {
        v[4 * k] = e2f<kH>(u[k].x); v[4 * k + 1] = e2f_hi<kH>(u[k].x);
        v[4 * k + 2] = e2f<kH>(u[k].y); v[4 * k + 3] = e2f_hi<kH>(u[k].y);
      } else {
        v[4 * k] = u[k].x; v[4 * k + 1] = u[k].y; v[4 * k + 2] = u[k].z; v[4 * k + 3] = u[k].w;
      }
    }
  }
};

GP_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

GP_DEV int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// kY: the add (y present); kLN: the LayerNorm; kIn16: the input x is 16-bit (LN only).
template <int EPL, bool kH, bool kY, bool kLN, bool kIn16>
__global__ __launch_bounds__(256) void rows_fwd_kernel(const void* x, const uint16_t* y, RowDrop d, const float* ln_w,
                                                       const float* ln_b, float eps, float* r, uint16_t* a,
                                                       uint32_t nrows) {
  static_assert(kY || kLN, "");
  static_assert(!(kY && kIn16), "");
  constexpr int C = 64 * EPL;
  const int lane = threadIdx.x & 63;
  // rows < 2^31 (host check): 32-bit row indices, 64-bit row offsets
  uint32_t row = blockIdx.x * 4 + wave_index();
  const uint32_t stride = gridDim.x * 4;
  if (row >= nrows) return;
  float w[kLN ? EPL : 1], b[kLN ? EPL : 1];
  if constexpr (kLN) {
    ld_x4_f32<EPL>(ln_w, lane, w);
    ld_x4_f32<EPL>(ln_b, lane, b);
  }
  RowRegs<EPL, kIn16> nx;
  RowRegs<EPL, true> ny;
  nx.load(x, (size_t)row * C, lane);
  if constexpr (kY) ny.load(y, (size_t)row * C, lane);
  for (; row < nrows; row += stride) {
    float v[EPL], yv[kY ? EPL : 1];
    nx.template unpack<kH>(v);
    if constexpr (kY) ny.template unpack<kH>(yv);
    // the next row of this wave; past the end the last row again (dropped when the loop ends)
    const uint32_t nrow = row + stride < nrows ? row + stride : nrows - 1;
    nx.load(x, (size_t)nrow * C, lane);
    if constexpr (kY) ny.load(y, (size_t)nrow * C, lane);
    if constexpr (kY) {
      float f[EPL];
      row_factors<EPL>(d, row, lane, f);
      row_add<EPL>(v, yv, f);
      st_x4_f32<EPL>(r + (size_t)row * C, lane, v);
    }
    if constexpr (kLN) {
      float mean, rstd;
      row_ln_stats<EPL>(v, eps, mean, rstd);
      row_ln_store<EPL, kH>(v, mean, rstd, w, b, a + (size_t)row * C, lane);
    }
  }
}

// kY: dy wanted (the forward had y); kLN: the forward had the LayerNorm (da, the saved LN input and ln_w given);
// kIn16: the saved input and dx are 16-bit; kDr: dr_in given; kParam: the dln_w / dln_b partials wanted.
template <int EPL, bool kH, bool kY, bool kLN, bool kIn16, bool kDr, bool kParam>
__global__ __launch_bounds__(256) void rows_bwd_kernel(const uint16_t* da, const float* dr_in, const void* saved,
                                                       const float* ln_w, float eps, RowDrop d, void* dx,
                                                       uint16_t* dy, float* __restrict__ part, uint32_t nrows) {
  static_assert(kLN || (kY && kDr && !kParam && !kIn16), "");
  static_assert(!(kY && kIn16), "");
  constexpr int C = 64 * EPL;
  constexpr int NA = kParam ? EPL : 1;
  const int lane = threadIdx.x & 63, wave = wave_index();
  uint32_t row = blockIdx.x * 4 + wave;
  const uint32_t stride = gridDim.x * 4;
  float w[kLN ? EPL : 1];
  if constexpr (kLN) ld_x4_f32<EPL>(ln_w, lane, w);
  // dln_w's terms da xhat are formed and summed in double, xhat from the row's statistics in double: a few rows'
  // worth of fp32 roundings would otherwise be the whole error of a short sum.  dln_b's terms are da itself.
  double aw[NA];
  float ab[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    aw[i] = 0.0;
    ab[i] = 0.f;
  }
  RowRegs<EPL, kIn16> nv;
  RowRegs<EPL, true> ng;
  RowRegs<EPL, false> nr;
  {
    // a wave without rows loads the last row and drops it (no early exit: the block meets at the barriers below)
    const size_t off = (size_t)(row < nrows ? row : nrows - 1) * C;
    if constexpr (kLN) {
      nv.load(saved, off, lane);
      ng.load(da, off, lane);
    }
    if constexpr (kDr) nr.load(dr_in, off, lane);
  }
  for (; row < nrows; row += stride) {
    float v[kLN ? EPL : 1], g[kLN ? EPL : 1], o[EPL];
    if constexpr (kLN) {
      nv.template unpack<kH>(v);
      ng.template unpack<kH>(g);
    }
    if constexpr (kDr) nr.template unpack<kH>(o);
    const uint32_t nrow = row + stride < nrows ? row + stride : nrows - 1;
    if constexpr (kLN) {
      nv.load(saved, (size_t)nrow * C, lane);
      ng.load(da, (size_t)nrow * C, lane);
    }
    if constexpr (kDr) nr.load(dr_in, (size_t)nrow * C, lane);
    if constexpr (kLN) {
      float mean, rstd;
      row_ln_stats<EPL>(v, eps, mean, rstd);
      if constexpr (kParam) {
        // the row's statistics once more in double, for dln_w alone (dx keeps the forward's fp32 mean / rstd)
        double sd = 0.0, qd = 0.0;
#pragma unroll
        for (int i = 0; i < EPL; ++i) sd += (double)v[i];
        const double md = wave_sum_f64(sd) / (double)C;
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
          const double t = (double)v[i] - md;
          qd = fma(t, t, qd);
        }
        const double rd = 1.0 / sqrt(wave_sum_f64(qd) / (double)C + (double)eps);
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
          aw[i] = fma((double)g[i], ((double)v[i] - md) * rd, aw[i]);
          ab[i] += g[i];
        }
      }
      float c1 = 0.f, c2 = 0.f;
#pragma unroll
      for (int i = 0; i < EPL; ++i) {
        v[i] = (v[i] - mean) * rstd;                 // xhat
        const float dxh = g[i] * w[i];
        c1 += dxh;
        c2 = fmaf(dxh, v[i], c2);
      }
      c1 = wave_sum(c1) / (float)C;
      c2 = wave_sum(c2) / (float)C;
#pragma unroll
      for (int i = 0; i < EPL; ++i) {
        // three roundings from da to dx: dxhat - c1, - xhat c2, dr_in + rstd (.)
        const float u = fmaf(-v[i], c2, fmaf(g[i], w[i], -c1));
        if constexpr (kDr) o[i] = fmaf(rstd, u, o[i]);
        else o[i] = rstd * u;
      }
    }
    if constexpr (kIn16) {
      st_x4_e<kH, EPL>(static_cast<uint16_t*>(dx) + (size_t)row * C, lane, o);
    } else {
      // (B) with dx == dr_in or without dx: the gradient of x is dr_in itself, nothing to write
      if (kLN || (dx != nullptr && dx != (const void*)dr_in)) st_x4_f32<EPL>(static_cast<float*>(dx) + (size_t)row * C, lane, o);
    }
    if constexpr (kY) {
      float f[EPL];
      row_factors<EPL>(d, row, lane, f);
#pragma unroll
      for (int i = 0; i < EPL; ++i) o[i] *= f[i];
      st_x4_e<kH, EPL>(dy + (size_t)row * C, lane, o);
    }
  }
  if constexpr (kParam) {
    __shared__ __attribute__((aligned(16))) float sp[2 * C];
#pragma unroll 1
    for (int wv = 0; wv < 4; ++wv) {
      if (wave == wv) {
#pragma unroll
        for (int k = 0; k < EPL / 4; ++k) {
          float4* pw = reinterpret_cast<float4*>(sp + k * 256 + 4 * lane);
          float4* pb = reinterpret_cast<float4*>(sp + C + k * 256 + 4 * lane);
          float4 sw = make_float4((float)aw[4 * k], (float)aw[4 * k + 1], (float)aw[4 * k + 2], (float)aw[4 * k + 3]);
          float4 sb = make_float4(ab[4 * k], ab[4 * k + 1], ab[4 * k + 2], ab[4 * k + 3]);
          if (wv > 0) {
            const float4 ow = *pw, ob = *pb;
            sw = make_float4(ow.x + sw.x, ow.y + sw.y, ow.z + sw.z, ow.w + sw.w);
            sb = make_float4(ob.x + sb.x, ob.y + sb.y, ob.z + sb.z, ob.w + sb.w);
          }
          *pw = sw;
          *pb = sb;
        }
      }
      __syncthreads();
    }
    float* dst = part + (size_t)blockIdx.x * 2 * C;
    for (int i = threadIdx.x * 4; i < 2 * C; i += 256 * 4)
      *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(sp + i);
  }
}

// dln_w[c] = sum over blocks of part[b][0][c], dln_b[c] likewise of part[b][1][c], in block order.
__global__ __launch_bounds__(64) void rows_bwd_reduce_kernel(const float* __restrict__ part, int nb, int C,
                                                             float* __restrict__ dln_w, float* __restrict__ dln_b) {
  const int i = blockIdx.x * 64 + threadIdx.x;        // [0, 2C)
  if (i >= 2 * C) return;
  // in double, rounded once: up to 1024 partials in sequence would otherwise cost more than the rows' own rounding
  double s = 0.0;
#pragma unroll 8
  for (int b = 0; b < nb; ++b) s += (double)part[(size_t)b * 2 * C + i];
  if (i < C) dln_w[i] = (float)s;
  else dln_b[i - C] = (float)s;
}

// out[4 q + j] = keep ? 1 : 0 for q < nquads, one quad per thread, grid-stride
__global__ __launch_bounds__(256) void keep_mask_kernel(uint32_t k0, uint32_t k1, uint32_t thr, uint64_t nquads,
                                                        uint32_t* __restrict__ out) {
  const uint64_t step = (uint64_t)gridDim.x * 256;
  for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < nquads; q += step) {
    bool keep[4] = {true, true, true, true};
    if (thr != 0) drop_keep4(k0, k1, thr, q, keep);
    out[q] = (uint32_t)keep[0] | ((uint32_t)keep[1] << 8) | ((uint32_t)keep[2] << 16) | ((uint32_t)keep[3] << 24);
  }
}

bool rows_cols_ok(int cols) { return cols == 768 || cols == 1024 || cols == 1536; }

int64_t rows_bwd_blocks(int64_t rows) {
  const int64_t want = (rows + 3) / 4;
  return want < kRowsBwdMaxBlocks ? want : kRowsBwdMaxBlocks;
}

bool overlaps(const void* p, uintptr_t np, const void* q, uintptr_t nq) {
  if (!p || !q) return false;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}

// the checks of p / s / rows_per_scale shared by both directions; fills d
int make_drop(const char* who, const float* s, int64_t rows_per_scale, float p, uint64_t seed, int64_t rows,
              RowDrop* d) {
  GP_REQUIRE(p >= 0.f && p < 1.f, "%s: p=%g outside [0, 1)", who, (double)p);
  if (s) {
    GP_REQUIRE(rows_per_scale > 0, "%s: rows_per_scale=%lld must be positive with s given", who,
               (long long)rows_per_scale);
    GP_REQUIRE(rows % rows_per_scale == 0, "%s: rows=%lld is no multiple of rows_per_scale=%lld", who,
               (long long)rows, (long long)rows_per_scale);
    GP_REQUIRE(gp_aligned(s, 4), "%s: misaligned s", who);
  }
  d->s = s;
  d->rps = s ? (uint32_t)rows_per_scale : 1u;
  d->thr = (uint32_t)((double)p * 4294967296.0);
  d->inv = 1.0f / (1.0f - p);
  d->k0 = (uint32_t)seed;
  d->k1 = (uint32_t)(seed >> 32);
  return 0;
}

}  // namespace

extern "C" size_t gp_resid_drop_ln_bwd_workspace_bytes(int64_t rows, int cols) {
  if (rows <= 0 || !rows_cols_ok(cols)) return 0;
  return (size_t)rows_bwd_blocks(rows) * 2 * (size_t)cols * sizeof(float);
}

extern "C" int gp_resid_drop_ln_fwd(const void* x, int x_is_act, const uint16_t* y, const float* s,
                                    int64_t rows_per_scale, float p, uint64_t seed, const float* ln_w,
                                    const float* ln_b, float eps, float* r, uint16_t* a, int64_t rows, int cols,
                                    int fmt, void* stream) {
  const char* who = "gp_resid_drop_ln_fwd";
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16, "%s: bad fmt %d", who, fmt);
  GP_REQUIRE(rows_cols_ok(cols), "%s: cols=%d unsupported (768, 1024, 1536)", who, cols);
  GP_REQUIRE(rows >= 0, "%s: bad rows", who);
  GP_REQUIRE(rows < (int64_t)0x7fffffff, "%s: too many rows", who);
  RowDrop d;
  if (int rc = make_drop(who, s, rows_per_scale, p, seed, rows, &d)) return rc;
  if (rows == 0) return 0;
  const bool add = y != nullptr, ln = ln_w != nullptr;
  GP_REQUIRE(x, "%s: null pointer (x)", who);
  GP_REQUIRE(add || ln, "%s: neither y nor ln_w given", who);
  GP_REQUIRE((ln_b != nullptr) == ln && (a != nullptr) == ln,
             "%s: ln_w, ln_b and a must all be given or all be null", who);
  GP_REQUIRE((r != nullptr) == add, "%s: r must be given with y and null without it", who);
  GP_REQUIRE(!(add && x_is_act), "%s: a 16-bit x is for the LayerNorm alone (y must be null)", who);
  GP_REQUIRE(gp_aligned(x, 16) && gp_aligned(y, 16) && gp_aligned(r, 16) && gp_aligned(a, 16) &&
             gp_aligned(ln_w, 16) && gp_aligned(ln_b, 16), "%s: misaligned pointer (16 bytes)", who);
  const uintptr_t n = (uintptr_t)rows * (uintptr_t)cols, nx = n * (x_is_act ? 2 : 4);
  GP_REQUIRE((const void*)r == x || !overlaps(r, n * 4, x, nx), "%s: r may alias x only as the same buffer", who);
  GP_REQUIRE(!overlaps(r, n * 4, y, n * 2) && !overlaps(r, n * 4, a, n * 2) && !overlaps(a, n * 2, x, nx) &&
             !overlaps(a, n * 2, y, n * 2), "%s: forbidden aliasing (only r over x is allowed)", who);
  const int64_t want = (rows + 3) / 4;
  const unsigned nb = (unsigned)(want < kRowsFwdMaxBlocks ? want : kRowsFwdMaxBlocks);
  hipStream_t st = gp_stream(stream);
  const uint32_t nrows = (uint32_t)rows;
#define GP_RF(EPL, KH, KY, KLN, K16) \
  rows_fwd_kernel<EPL, KH, KY, KLN, K16><<<nb, 256, 0, st>>>(x, y, d, ln_w, ln_b, eps, r, a, nrows)
#define GP_RF_SHAPE(EPL, KH)                          \
  do {                                                \
    if (add && ln) GP_RF(EPL, KH, true, true, false); \
    else if (add) GP_RF(EPL, KH, true, false, false); \
    else if (x_is_act) GP_RF(EPL, KH, false, true, true); \
    else GP_RF(EPL, KH, false, true, false);          \
  } while (0)
#define GP_RF_FMT(EPL) \
  do { if (fmt == GP_FMT_F16) GP_RF_SHAPE(EPL, true); else GP_RF_SHAPE(EPL, false); } while (0)
  switch (cols / 64) {
    case 12: GP_RF_FMT(12); break;
    case 16: GP_RF_FMT(16); break;
    case 24: GP_RF_FMT(24); break;
  }
#undef GP_RF_FMT
#undef GP_RF_SHAPE
#undef GP_RF
  return gp_check_launch(who);
}

extern "C" int gp_resid_drop_ln_bwd(const uint16_t* da, const float* dr_in, const void* saved, int saved_is_act,
                                    const float* ln_w, float eps, const float* s, int64_t rows_per_scale, float p,
                                    uint64_t seed, void* dx, uint16_t* dy, float* dln_w, float* dln_b,
                                    void* workspace, size_t workspace_bytes, int64_t rows, int cols, int fmt,
                                    void* stream) {
  const char* who = "gp_resid_drop_ln_bwd";
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16, "%s: bad fmt %d", who, fmt);
  GP_REQUIRE(rows_cols_ok(cols), "%s: cols=%d unsupported (768, 1024, 1536)", who, cols);
  GP_REQUIRE(rows >= 0, "%s: bad rows", who);
  GP_REQUIRE(rows < (int64_t)0x7fffffff, "%s: too many rows", who);
  RowDrop d;
  if (int rc = make_drop(who, s, rows_per_scale, p, seed, rows, &d)) return rc;
  GP_REQUIRE((dln_w == nullptr) == (dln_b == nullptr), "%s: dln_w and dln_b must both be given or both be null", who);
  if (rows == 0) return 0;
  const bool ln = ln_w != nullptr, add = dy != nullptr, in16 = saved_is_act != 0, dr = dr_in != nullptr;
  const bool param = dln_w != nullptr;
  GP_REQUIRE(ln || add, "%s: neither ln_w nor dy given", who);
  if (ln) {
    GP_REQUIRE(da && saved && dx, "%s: null pointer (da, saved and dx go with ln_w)", who);
  } else {
    GP_REQUIRE(!da && !saved && !param, "%s: da, saved and dln_* must be null without ln_w", who);
    GP_REQUIRE(dr, "%s: null pointer (dr_in is the only gradient without ln_w)", who);
  }
  GP_REQUIRE(!(add && in16), "%s: a 16-bit saved input is for the LayerNorm alone (dy must be null)", who);
  GP_REQUIRE(gp_aligned(da, 16) && gp_aligned(dr_in, 16) && gp_aligned(saved, 16) && gp_aligned(ln_w, 16) &&
             gp_aligned(dx, 16) && gp_aligned(dy, 16) && gp_aligned(dln_w, 4) && gp_aligned(dln_b, 4),
             "%s: misaligned pointer (16 bytes)", who);
  const uintptr_t n = (uintptr_t)rows * (uintptr_t)cols, nsv = n * (in16 ? 2 : 4), ndx = nsv;
  GP_REQUIRE((const void*)dx == (const void*)dr_in || !overlaps(dx, ndx, dr_in, n * 4),
             "%s: dx may alias dr_in only as the same buffer", who);
  GP_REQUIRE(!(in16 && dx && (const void*)dx == (const void*)dr_in), "%s: a 16-bit dx cannot alias the fp32 dr_in", who);
  GP_REQUIRE(!overlaps(dx, ndx, da, n * 2) && !overlaps(dx, ndx, saved, nsv) && !overlaps(dx, ndx, dy, n * 2) &&
             !overlaps(dy, n * 2, da, n * 2) && !overlaps(dy, n * 2, saved, nsv) && !overlaps(dy, n * 2, dr_in, n * 4),
             "%s: forbidden aliasing (only dx over dr_in is allowed)", who);
  const unsigned nb = (unsigned)rows_bwd_blocks(rows);
  if (param) {
    const size_t need = gp_resid_drop_ln_bwd_workspace_bytes(rows, cols);
    GP_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu bytes, need %zu)", who,
               workspace ? workspace_bytes : (size_t)0, need);
    GP_REQUIRE(gp_aligned(workspace, 16), "%s: misaligned workspace", who);
  }
  hipStream_t st = gp_stream(stream);
  float* part = static_cast<float*>(workspace);
  const uint32_t nrows = (uint32_t)rows;
#define GP_RB(EPL, KH, KY, KLN, K16, KDR, KP) \
  rows_bwd_kernel<EPL, KH, KY, KLN, K16, KDR, KP><<<nb, 256, 0, st>>>(da, dr_in, saved, ln_w, eps, d, dx, dy, part, nrows)
#define GP_RB_P(EPL, KH, KY, K16, KDR) \
  do { if (param) GP_RB(EPL, KH, KY, true, K16, KDR, true); else GP_RB(EPL, KH, KY, true, K16, KDR, false); } while (0)
#define GP_RB_DR(EPL, KH, KY, K16) \
  do { if (dr) GP_RB_P(EPL, KH, KY, K16, true); else GP_RB_P(EPL, KH, KY, K16, false); } while (0)
#define GP_RB_SHAPE(EPL, KH)                                        \
  do {                                                              \
    if (!ln) GP_RB(EPL, KH, true, false, false, true, false);       \
    else if (add) GP_RB_DR(EPL, KH, true, false);                   \
    else if (in16) GP_RB_DR(EPL, KH, false, true);                  \
    else GP_RB_DR(EPL, KH, false, false);                           \
  } while (0)
#define GP_RB_FMT(EPL) \
  do { if (fmt == GP_FMT_F16) GP_RB_SHAPE(EPL, true); else GP_RB_SHAPE(EPL, false); } while (0)
  switch (cols / 64) {
    case 12: GP_RB_FMT(12); break;
    case 16: GP_RB_FMT(16); break;
    case 24: GP_RB_FMT(24); break;
  }
#undef GP_RB_FMT
#undef GP_RB_SHAPE
#undef GP_RB_DR
#undef GP_RB_P
#undef GP_RB
  if (param)
    rows_bwd_reduce_kernel<<<(unsigned)(2 * cols / 64), 64, 0, st>>>(part, (int)nb, cols, dln_w, dln_b);
  return gp_check_launch(who);
}

extern "C" int gp_dropout_keep_mask(uint64_t seed, float p, int64_t rows, int cols, uint8_t* out, void* stream) {
  const char* who = "gp_dropout_keep_mask";
  GP_REQUIRE(p >= 0.f && p < 1.f, "%s: p=%g outside [0, 1)", who, (double)p);
  GP_REQUIRE(cols > 0 && cols % 4 == 0, "%s: cols=%d must be a positive multiple of 4", who, cols);
  GP_REQUIRE(rows >= 0, "%s: bad rows", who);
  GP_REQUIRE(rows < (int64_t)0x7fffffff, "%s: too many rows", who);
  if (rows == 0) return 0;
  GP_REQUIRE(out, "%s: null pointer", who);
  GP_REQUIRE(gp_aligned(out, 4), "%s: misaligned pointer (4 bytes)", who);
  const uint64_t nquads = (uint64_t)rows * (uint64_t)(cols / 4);
  const uint64_t want = (nquads + 255) / 256;
  const unsigned nb = (unsigned)(want < 4096 ? want : 4096);
  keep_mask_kernel<<<nb, 256, 0, gp_stream(stream)>>>((uint32_t)seed, (uint32_t)(seed >> 32),
                                                      (uint32_t)((double)p * 4294967296.0), nquads,
                                                      reinterpret_cast<uint32_t*>(out));
  return gp_check_launch(who);
}
