// Backward of the FFN's GELU + LayerNorm (gp_gelu_layernorm_bwd): a translation unit of its own, so that the code
// object of the forward row kernels (gp_norm.hip) is not touched by it.
#include <math.h>
#include <stdlib.h>

#include "gp_api.h"
#include "gp_common.h"

namespace {

// gelu_erf of gp_norm.hip (the forward's arithmetic: g is recomputed with it, bit for bit):
// Exact-erf GELU, x * Phi(x) = 0.5 x (1 + erf(x / sqrt 2)) (feedforward_network.py:135, torch's
// F.gelu default), with erf from Abramowitz & Stegun 7.1.26: |erf error| <= 1.5e-7, i.e. GELU
// within 0.75e-7 |x| of the libm value -- far below the bf16 rounding of the output, at a
// fraction of erff's instruction count (one v_rcp, one v_exp, ~10 FMA-class ops).
GP_DEV float gelu_erf(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  float poly = fmaf(1.061405429f, t, -1.453152027f);
  poly = fmaf(poly, t, 1.421413741f);
  poly = fmaf(poly, t, -0.284496736f);
  poly = fmaf(poly, t, 0.254829592f);
  poly *= t;
  const float e = __builtin_amdgcn_exp2f(-z * z * 1.44269504088896340736f);
  const float erf_x = copysignf(fmaf(-poly, e, 1.0f), x);
  const float hx = 0.5f * x;
  return fmaf(hx, erf_x, hx);
}

// ---------------------------------------------------------------------------------------
// Backward of GELU + LN (y = LN(round(gelu_erf(h))) w + b).  Nothing but h is saved by the forward:
// g = round(gelu_erf(h)) and the LN statistics are recomputed with the forward's arithmetic, then
//   dxhat = dy w,  dg = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)),  dh = round(dg gelu'(h))
// with gelu'(h) = 0.5 (1 + erf(h / sqrt 2)) + h exp(-h^2 / 2) / sqrt(2 pi) from the same A&S 7.1.26 pieces as
// gelu_erf (the rounding of g is straight-through).
// Layout: a block of 4 waves walks groups of R rows grid-stride, every thread owning the same EPT = cols / 256
// columns (k * 1024 + 4 * tid + {0..3}) of each row of the group, with the next group's h and dy loads issued
// before the current group's math and the LN weights in LDS.  The wave-per-row layout of the forward would keep
// 2 * cols / 64 per-lane column sums for dln_w / dln_b (192 registers at cols = 6144: scratch spills); here a
// thread keeps 2 * EPT, and the three row reductions (sum g; sum (g - mean)^2; sum dxhat and sum dxhat xhat) go
// wave butterfly -> LDS -> the four waves added in wave order, R rows per barrier.  A group's h and dy are in
// registers before its dh is stored, so dh may alias dy.
// kParam: each thread sums dy xhat and dy over the rows its block walks and the block writes one [2][C]
// partial; gelu_ln_bwd_reduce_kernel adds the partials in block order.  No atomics, and the grid is a function
// of (rows, cols) alone, so dln_w / dln_b are the same bits on every run and every device.
constexpr int kGeluBwdMaxBlocks = 1024;

GP_DEV float gelu_erf_grad(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  float poly = fmaf(1.061405429f, t, -1.453152027f);
  poly = fmaf(poly, t, 1.421413741f);
  poly = fmaf(poly, t, -0.284496736f);
  poly = fmaf(poly, t, 0.254829592f);
  poly *= t;
  const float e = __builtin_amdgcn_exp2f(-z * z * 1.44269504088896340736f);     // exp(-x^2 / 2)
  const float erf_x = copysignf(fmaf(-poly, e, 1.0f), x);
  return fmaf(x * e, 0.39894228040143267794f, fmaf(0.5f, erf_x, 0.5f));
}

template <bool kH>
GP_DEV void unpack4(const uint2 u, float* v) {
  v[0] = e2f<kH>(u.x);
  v[1] = e2f_hi<kH>(u.x);
  v[2] = e2f<kH>(u.y);
  v[3] = e2f_hi<kH>(u.y);
}
template <bool kH>
GP_DEV uint2 pack4(const float* v) {
  return make_uint2(pack2e<kH>(v[0], v[1]), pack2e<kH>(v[2], v[3]));
}

// Keeps a packed value packed: without it the compiler carries the unpacked fp32 values from one pass over the
// rows to the next (twice the registers) instead of unpacking again.
GP_DEV void keep_packed(uint2& u) { asm volatile("" : "+v"(u.x), "+v"(u.y)); }

// Sums of N per-thread values over the block's 256 threads, to every thread: wave butterfly, then the four
// waves' sums through red [4][N] in wave order.  One barrier; the caller alternates red between uses.
template <int N>
GP_DEV void block_sum4(float* v, float* red, int lane, int wave) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[wave * N + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = ((red[i] + red[N + i]) + red[2 * N + i]) + red[3 * N + i];
}

template <int EPT, int R, bool kH, bool kParam>
__global__ __launch_bounds__(256, 2) void gelu_ln_bwd_kernel(const uint16_t* h, const uint16_t* dy,
                                                             const float* __restrict__ ln_w, float eps,
                                                             uint16_t* dh, float* __restrict__ part,
                                                             int64_t rows) {
  constexpr int C = 256 * EPT, NK = EPT / 4;
  constexpr int NA = kParam ? EPT : 1;
  __shared__ __attribute__((aligned(16))) float sw[C];
  // one slot per reduction of an iteration: a slot is rewritten two barriers after its last read
  __shared__ float red[3][4 * 2 * R];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t toff = 4u * (uint32_t)tid;      // the thread's column offset: row bases stay scalar
  for (int i = tid * 4; i < C; i += 256 * 4)
    *reinterpret_cast<float4*>(sw + i) = *reinterpret_cast<const float4*>(ln_w + i);
  __syncthreads();
  // rows < 2^31 (host check): row indices are 32-bit scalars, the row base a scalar 64-bit product
  const uint32_t nrows = (uint32_t)rows, stride = gridDim.x * R;
  float aw[NA], ab[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) aw[i] = ab[i] = 0.f;
  uint2 ch[R][NK], cd[R][NK], nh[R][NK], nd[R][NK];
  // a group's h and dy; a row past the end reads the last row's address and becomes zeros (g = 0, xhat = 0,
  // dy = 0: nothing added to the column sums, nothing stored).  The zeroing is a separate step: applied to the
  // prefetched group it would wait for the loads right after issuing them
  auto load_group = [&](uint32_t g, uint2 (&gh)[R][NK], uint2 (&gd)[R][NK]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const size_t base = (size_t)(g + r < nrows ? g + r : nrows - 1) * C;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        gh[r][k] = *reinterpret_cast<const uint2*>((h + (base + k * 1024)) + toff);
        gd[r][k] = *reinterpret_cast<const uint2*>((dy + (base + k * 1024)) + toff);
      }
    }
  };
  auto take_group = [&](uint32_t g, const uint2 (&gh)[R][NK], const uint2 (&gd)[R][NK]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool ok = g + r < nrows;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        ch[r][k] = ok ? gh[r][k] : make_uint2(0, 0);
        cd[r][k] = ok ? gd[r][k] : make_uint2(0, 0);
      }
    }
  };
  uint32_t g0 = blockIdx.x * R;
  if (g0 < nrows) {
    load_group(g0, nh, nd);
    take_group(g0, nh, nd);
  }
  for (; g0 < nrows; g0 += stride) {
    // unconditional (past the end it re-reads the last row, from the cache): under a branch the compiler copies
    // the loaded registers at once and waits for them
    load_group(g0 + stride, nh, nd);
    // g = round(gelu(h)), kept packed; the LN statistics over the rounded values (two passes, as the forward)
    uint2 cg[R][NK];
    float mean[R], rstd[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        float v[4];
        unpack4<kH>(ch[r][k], v);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = gelu_erf(v[i]);
        cg[r][k] = pack4<kH>(v);
        unpack4<kH>(cg[r][k], v);
#pragma unroll
        for (int i = 0; i < 4; ++i) s += v[i];
        __builtin_amdgcn_sched_barrier(0);   // one chunk's GELU temporaries live at a time
      }
      mean[r] = s;
    }
    block_sum4<R>(mean, red[0], lane, wave);
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        keep_packed(cg[r][k]);
        keep_packed(cd[r][k]);
        keep_packed(ch[r][k]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      mean[r] /= (float)C;
      float q = 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        float v[4];
        unpack4<kH>(cg[r][k], v);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float d = v[i] - mean[r];
          q += d * d;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      rstd[r] = q;
    }
    block_sum4<R>(rstd, red[1], lane, wave);
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        keep_packed(cg[r][k]);
        keep_packed(cd[r][k]);
        keep_packed(ch[r][k]);
      }
    }
    // c[r] = mean(dxhat), c[R + r] = mean(dxhat xhat)
    float c[2 * R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      rstd[r] = rsqrtf(rstd[r] / (float)C + eps);
      float c1 = 0.f, c2 = 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        float v[4], d[4];
        unpack4<kH>(cg[r][k], v);
        unpack4<kH>(cd[r][k], d);
        const float4 w4 = *reinterpret_cast<const float4*>((sw + k * 1024) + toff);
        const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float dx = d[i] * wv[i];
          c1 += dx;
          c2 += dx * ((v[i] - mean[r]) * rstd[r]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      c[r] = c1;
      c[R + r] = c2;
    }
    block_sum4<2 * R>(c, red[2], lane, wave);
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        keep_packed(cg[r][k]);
        keep_packed(cd[r][k]);
        keep_packed(ch[r][k]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float c1 = c[r] / (float)C, c2 = c[R + r] / (float)C;
      const bool ok = g0 + r < nrows;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        float v[4], d[4], x[4];
        unpack4<kH>(cg[r][k], v);
        unpack4<kH>(cd[r][k], d);
        unpack4<kH>(ch[r][k], x);
        const float4 w4 = *reinterpret_cast<const float4*>((sw + k * 1024) + toff);
        const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float xhat = (v[i] - mean[r]) * rstd[r];
          if constexpr (kParam) {
            aw[4 * k + i] = fmaf(d[i], xhat, aw[4 * k + i]);
            ab[4 * k + i] += d[i];
          }
          x[i] = rstd[r] * (d[i] * wv[i] - c1 - xhat * c2) * gelu_erf_grad(x[i]);
        }
        if (ok) *reinterpret_cast<uint2*>((dh + ((size_t)(g0 + r) * C + k * 1024)) + toff) = pack4<kH>(x);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    take_group(g0 + stride, nh, nd);
  }
  if constexpr (kParam) {
    float* dst = part + (size_t)blockIdx.x * 2 * C;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      *reinterpret_cast<float4*>(dst + k * 1024 + 4 * tid) =
          make_float4(aw[4 * k], aw[4 * k + 1], aw[4 * k + 2], aw[4 * k + 3]);
      *reinterpret_cast<float4*>(dst + C + k * 1024 + 4 * tid) =
          make_float4(ab[4 * k], ab[4 * k + 1], ab[4 * k + 2], ab[4 * k + 3]);
    }
  }
}

// dln_w[c] = sum over blocks of part[b][0][c], dln_b[c] likewise of part[b][1][c], in block order.
__global__ __launch_bounds__(64) void gelu_ln_bwd_reduce_kernel(const float* __restrict__ part, int nb, int C,
                                                                float* __restrict__ dln_w,
                                                                float* __restrict__ dln_b) {
  const int i = blockIdx.x * 64 + threadIdx.x;        // [0, 2C)
  if (i >= 2 * C) return;
  float s = 0.f;
#pragma unroll 8
  for (int b = 0; b < nb; ++b) s += part[(size_t)b * 2 * C + i];
  if (i < C) dln_w[i] = s;
  else dln_b[i - C] = s;
}

}  // namespace

// fmt: GP_FMT_BF16 or GP_FMT_F16
#define GP_FMT_DISPATCH(fmt, KERNEL_CALL_H, KERNEL_CALL_B) \
  do {                                                    \
    if (fmt == GP_FMT_F16) { KERNEL_CALL_H; } else { KERNEL_CALL_B; } \
  } while (0)

static bool gelu_cols_ok(int cols) {
  return cols % 64 == 0 && (cols / 64 == 48 || cols / 64 == 64 || cols / 64 == 96);
}
// rows a block of gelu_ln_bwd_kernel holds at a time, and its grid: functions of (rows, cols) alone
static int gelu_bwd_group(int cols) { return cols == 6144 ? 1 : 2; }
static int64_t gelu_bwd_blocks(int64_t rows, int cols) {
  const int r = gelu_bwd_group(cols);
  const int64_t want = (rows + r - 1) / r;
  return want < kGeluBwdMaxBlocks ? want : kGeluBwdMaxBlocks;
}

extern "C" size_t gp_gelu_layernorm_bwd_workspace_bytes(int64_t rows, int cols) {
  if (rows <= 0 || !gelu_cols_ok(cols)) return 0;
  return (size_t)gelu_bwd_blocks(rows, cols) * 2 * (size_t)cols * sizeof(float);
}

extern "C" int gp_gelu_layernorm_bwd(const uint16_t* h, const uint16_t* dy, const float* ln_w, float eps,
                                     uint16_t* dh, float* dln_w, float* dln_b, void* workspace,
                                     size_t workspace_bytes, int64_t rows, int cols, int fmt, void* stream) {
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16, "gp_gelu_layernorm_bwd: bad fmt %d", fmt);
  GP_REQUIRE(gelu_cols_ok(cols), "gp_gelu_layernorm_bwd: cols=%d unsupported (64*{48,64,96})", cols);
  GP_REQUIRE(rows >= 0, "gp_gelu_layernorm_bwd: bad rows");
  if (rows == 0) return 0;
  GP_REQUIRE(h && dy && ln_w && dh, "gp_gelu_layernorm_bwd: null pointer");
  GP_REQUIRE((dln_w == nullptr) == (dln_b == nullptr),
             "gp_gelu_layernorm_bwd: dln_w and dln_b must both be given or both be null");
  GP_REQUIRE(rows < (int64_t)0x7fffffff, "gp_gelu_layernorm_bwd: too many rows");
  GP_REQUIRE(gp_aligned(h, 16) && gp_aligned(dy, 16) && gp_aligned(dh, 16) && gp_aligned(ln_w, 16),
             "gp_gelu_layernorm_bwd: misaligned pointer (16 bytes)");
  const uintptr_t n16 = (uintptr_t)rows * (uintptr_t)cols * 2;
  const uintptr_t ph = (uintptr_t)h, pd = (uintptr_t)dy, po = (uintptr_t)dh;
  GP_REQUIRE(po + n16 <= ph || ph + n16 <= po, "gp_gelu_layernorm_bwd: dh must not alias h");
  GP_REQUIRE(po == pd || po + n16 <= pd || pd + n16 <= po,
             "gp_gelu_layernorm_bwd: dh may alias dy only as the same buffer");
  const unsigned nb = (unsigned)gelu_bwd_blocks(rows, cols);
  const bool param = dln_w != nullptr;
  if (param) {
    GP_REQUIRE(workspace && workspace_bytes >= gp_gelu_layernorm_bwd_workspace_bytes(rows, cols),
               "gp_gelu_layernorm_bwd: workspace too small (%zu bytes, need %zu)", workspace ? workspace_bytes : (size_t)0,
               gp_gelu_layernorm_bwd_workspace_bytes(rows, cols));
    GP_REQUIRE(gp_aligned(workspace, 16), "gp_gelu_layernorm_bwd: misaligned workspace");
  }
  hipStream_t s = gp_stream(stream);
  float* part = static_cast<float*>(workspace);
#define GP_GLB(EPT, R, KH, KP) gelu_ln_bwd_kernel<EPT, R, KH, KP><<<nb, 256, 0, s>>>(h, dy, ln_w, eps, dh, part, rows)
#define GP_GLB_FMT(EPT, R, KP) GP_FMT_DISPATCH(fmt, GP_GLB(EPT, R, true, KP), GP_GLB(EPT, R, false, KP))
  switch (cols / 256) {
    case 12: if (param) GP_GLB_FMT(12, 2, true); else GP_GLB_FMT(12, 2, false); break;
    case 16: if (param) GP_GLB_FMT(16, 2, true); else GP_GLB_FMT(16, 2, false); break;
    case 24: if (param) GP_GLB_FMT(24, 1, true); else GP_GLB_FMT(24, 1, false); break;
  }
#undef GP_GLB_FMT
#undef GP_GLB
  if (param)
    gelu_ln_bwd_reduce_kernel<<<(unsigned)(2 * cols / 64), 64, 0, s>>>(part, (int)nb, cols, dln_w, dln_b);
  return gp_check_launch("gp_gelu_layernorm_bwd");
}
