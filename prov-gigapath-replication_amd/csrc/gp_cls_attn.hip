// gp_cls_attn_merge_ln: the CLS token's row of DilatedAttention.forward (dilated_attention.py:133-217) for
// the last encoder layer, whose only consumer is the CLS readout (slide_encoder.py:213-221).  Two launches,
// no atomics, flags or inter-block waits:
//   1. cls_attn_partial_kernel: grid (work item, slide), work item = (branch, covered head, 256-key chunk).
//      One key per thread: fp32 q.k, the chunk's log2-domain max, sum of exp2 and sum of exp2 * v, written
//      to the workspace as one (max, sum, acc[D]) record.
//   2. cls_merge_ln_kernel: one workgroup per slide.  Combines the chunks of every (branch, head) into
//      o (rounded to the activation format, as the per-branch o buffers of gp_dilated_attn_fwd are) and the
//      natural-log LSE, merges the branches (dilated_attention.py:100-131) and applies inner_attn_ln.
// Geometry (header comment of the entry in include/gigapath_hip.h): the CLS token is sparse row 0 of
// segment 0, phase 0 of every branch, so only heads h < hpg are covered and its keys are tokens
// 0, r, 2r, ..., (m - 1) r -- all real tokens, no zero-pad keys.
#include <math.h>

#include <algorithm>

#include "gp_api.h"
#include "gp_common.h"

namespace {

constexpr int kChunk = 256;        // keys per work item = threads per workgroup
constexpr int kRecHead = 4;        // record: max, sum, 2 pad floats, then acc[D] (16-byte aligned)

struct ClsArgs {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  int64_t row_stride;
  const int64_t* slide_off;
  const int64_t* slide_len;
  int64_t max_len;
  int32_t H, D, nbranch, items;    // items: records per slide = sum_b hpg_b * mc_b
  int32_t sl[GP_MAX_BRANCHES];
  int32_t r[GP_MAX_BRANCHES];
  int32_t hpg[GP_MAX_BRANCHES];    // covered heads (heads per dilation group)
  int32_t mc[GP_MAX_BRANCHES];     // chunks of the branch at max_len
  int32_t pre[GP_MAX_BRANCHES + 1];   // first record of the branch
  float qk_scale;                  // log2-domain logits = q.k * qk_scale
  const float* ln_w;
  const float* ln_b;
  float eps;
  uint16_t* out;
  float* ws;
  // compact K / V rows (gp_cls_attn_merge_ln_map): token t of a slide lies at row slide_off + row_map[t], and the
  // slide holds map_rows rows; NULL: at row slide_off + t
  const int32_t* row_map;
  int32_t map_rows;
};

// sparse rows (= keys of the CLS query) of branch b at slide length L
GP_DEV int cls_keys(const ClsArgs& a, int b, int64_t L) {
  const int64_t s = a.sl[b] < L ? (int64_t)a.sl[b] : L;
  return (int)((s + a.r[b] - 1) / a.r[b]);
}
GP_DEV int64_t cls_len(const ClsArgs& a, int slide) {
  const int64_t L = a.slide_len[slide];
  return L < 1 ? 1 : (L > a.max_len ? a.max_len : L);   // (records and keys stay inside what the host sized)
}

template <bool kH16>
GP_DEV void unpack8(const uint4 u, float* out) {        // 8 16-bit values of one 16-byte access
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    out[2 * j] = e2f<kH16>(w[j] & 0xffffu);
    out[2 * j + 1] = e2f_hi<kH16>(w[j]);
  }
}

// kQK / kV: q and k / v are fp16 (else bf16)
template <int D, bool kQK, bool kV>
__global__ __launch_bounds__(kChunk) void cls_attn_partial_kernel(const ClsArgs a) {
  __shared__ float red[4][D + 2];
  const int slide = blockIdx.y;
  int item = blockIdx.x, b = 0;
  while (b + 1 < a.nbranch && item >= a.pre[b + 1]) ++b;
  item -= a.pre[b];
  const int h = item / a.mc[b];
  const int c = item - h * a.mc[b];
  const int64_t L = cls_len(a, slide);
  const int m = cls_keys(a, b, L);
  const int k0 = c * kChunk;
  if (k0 >= m) return;                                   // (workgroup-uniform)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool valid = k0 + tid < m;
  const int64_t tok0 = a.slide_off[slide];
  int64_t trow = valid ? (int64_t)(k0 + tid) * a.r[b] : 0;
  if (a.row_map != nullptr) {                            // (held inside the slide's rows whatever the map says)
    const int32_t mr = a.row_map[trow];
    trow = mr < 0 ? 0 : (mr < a.map_rows ? mr : a.map_rows - 1);
  }
  const int64_t tok = tok0 + trow;
  // the key's k and v rows (D 16-bit values each, 16-byte accesses), all in flight before the first use
  const uint4* kp = reinterpret_cast<const uint4*>(a.k + tok * a.row_stride + h * D);
  const uint4* vp = reinterpret_cast<const uint4*>(a.v + tok * a.row_stride + h * D);
  const uint4* qp = reinterpret_cast<const uint4*>(a.q + tok0 * a.row_stride + h * D);
  uint4 kr[D / 8], vr[D / 8];
#pragma unroll
  for (int i = 0; i < D / 8; ++i) kr[i] = kp[i];
#pragma unroll
  for (int i = 0; i < D / 8; ++i) vr[i] = vp[i];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < D / 8; ++i) {
    float qf[8], kf[8];
    unpack8<kQK>(qp[i], qf);
    unpack8<kQK>(kr[i], kf);
#pragma unroll
    for (int j = 0; j < 8; ++j) dot = __builtin_fmaf(qf[j], kf[j], dot);
  }
  const float s2 = valid ? dot * a.qk_scale : -INFINITY;
  float mx = wave_max(s2);
  if (lane == 0) red[wv][0] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
  const float p = valid ? exp2f(s2 - mx) : 0.f;
  const float ps = wave_sum(p);
#pragma unroll
  for (int i = 0; i < D / 8; ++i) {
    float vf[8];
    unpack8<kV>(vr[i], vf);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float t = wave_sum(valid ? p * vf[j] : 0.f);  // (an unused lane's v row is never multiplied)
      if (lane == 0) red[wv][2 + 8 * i + j] = t;
    }
  }
  if (lane == 0) red[wv][1] = ps;
  __syncthreads();
  float* rec = a.ws + ((int64_t)slide * a.items + blockIdx.x) * (D + kRecHead);
  if (tid < D) rec[kRecHead + tid] = (red[0][2 + tid] + red[1][2 + tid]) + (red[2][2 + tid] + red[3][2 + tid]);
  if (tid == D) rec[0] = mx;
  if (tid == D + 1) rec[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
}

constexpr int kMergeWaves = 16;    // waves of the per-slide workgroup: one (branch, head) each per round

GP_DEV float block_sum(float v, float* red, int tid) {   // red: kMergeWaves floats
  v = wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < kMergeWaves; ++w) t += red[w];
  return t;
}

template <bool kH>
__global__ __launch_bounds__(64 * kMergeWaves) void cls_merge_ln_kernel(const ClsArgs a) {
  extern __shared__ float smem[];
  const int H = a.H, D = a.D, E = H * D, nbr = a.nbranch;
  float* o_s = smem;                     // [nbranch][H][D] rounded o of the covered (branch, head)
  float* lse_s = smem + nbr * E;         // [nbranch][H]
  float* red = lse_s + nbr * H;          // [kMergeWaves]
  const int slide = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t L = cls_len(a, slide);
  const int rs = D + kRecHead;
  int pair = 0;
  for (int b = 0; b < nbr; ++b) {
    const int nch = (cls_keys(a, b, L) + kChunk - 1) / kChunk;
    for (int h = 0; h < a.hpg[b]; ++h, ++pair) {
      if (pair % kMergeWaves != wv) continue;            // one wave per (branch, head)
      // the chunks' (max, sum, acc[D]) records -> softmax over all keys: lane c holds chunk c's factor
      // exp2(max_c - max), lanes d and d + 64 accumulate columns d, d + 64 of sum_c factor_c * acc_c
      const float* rec = a.ws + ((int64_t)slide * a.items + a.pre[b] + h * a.mc[b]) * rs;
      float mx = -INFINITY;
      for (int c = lane; c < nch; c += 64) mx = fmaxf(mx, rec[c * rs]);
      mx = wave_max(mx);
      float sum = 0.f, acc0 = 0.f, acc1 = 0.f;
      for (int c0 = 0; c0 < nch; c0 += 64) {
        const int c = c0 + lane;
        const float f = c < nch ? exp2f(rec[c * rs] - mx) : 0.f;
        if (c < nch) sum = __builtin_fmaf(rec[c * rs + 1], f, sum);
        const int n = nch - c0 < 64 ? nch - c0 : 64;
        for (int cc = 0; cc < n; cc += 8) {              // 8 chunks' loads in flight (past n: factor 0)
          float x0[8], x1[8], fc[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int ci = cc + j < n ? cc + j : n - 1;
            const float* r = rec + (c0 + ci) * rs + kRecHead;
            x0[j] = lane < D ? r[lane] : 0.f;
            x1[j] = lane + 64 < D ? r[lane + 64] : 0.f;
            const float fj = __shfl(f, ci, 64);
            fc[j] = cc + j < n ? fj : 0.f;
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            acc0 = __builtin_fmaf(x0[j], fc[j], acc0);
            acc1 = __builtin_fmaf(x1[j], fc[j], acc1);
          }
        }
      }
      sum = wave_sum(sum);
      if (lane < D) o_s[(b * H + h) * D + lane] = e2f<kH>(f2e<kH>(acc0 / sum));
      if (lane + 64 < D) o_s[(b * H + h) * D + lane + 64] = e2f<kH>(f2e<kH>(acc1 / sum));
      if (lane == 0) lse_s[b * H + h] = (mx + log2f(sum)) * 0.69314718055994530942f;
    }
  }
  __syncthreads();
  // merge (dilated_attention.py:100-131): fp32 softmax over ALL branches' LSEs (uncovered: -1e8, lse == 0 ->
  // -1e8, :46), weighted sum in branch order; two adjacent columns per thread
  constexpr int kMaxPairs = 1;           // two columns per thread: E <= 2048
  constexpr int kStep = 128 * kMergeWaves;
  float val[kMaxPairs][2];
  float part = 0.f;
#pragma unroll
  for (int i = 0; i < kMaxPairs; ++i) {
    const int e = 2 * tid + i * kStep;
    val[i][0] = val[i][1] = 0.f;
    if (e < E) {
      const int h = e / D;
      float lse[GP_MAX_BRANCHES];
      float mx = -INFINITY;
#pragma unroll
      for (int b = 0; b < GP_MAX_BRANCHES; ++b) {
        float l = (b < nbr && h < a.hpg[b]) ? lse_s[b * H + h] : -1e8f;
        if (l == 0.f) l = -1e8f;
        lse[b] = l;
        if (b < nbr) mx = fmaxf(mx, l);
      }
      float wsum = 0.f;
#pragma unroll
      for (int b = 0; b < GP_MAX_BRANCHES; ++b)
        if (b < nbr) {
          lse[b] = expf(lse[b] - mx);
          wsum += lse[b];
        }
#pragma unroll
      for (int b = 0; b < GP_MAX_BRANCHES; ++b)
        if (b < nbr && h < a.hpg[b]) {
          const float w = lse[b] / wsum;
          val[i][0] = __builtin_fmaf(o_s[b * E + e], w, val[i][0]);
          val[i][1] = __builtin_fmaf(o_s[b * E + e + 1], w, val[i][1]);
        }
      part += val[i][0] + val[i][1];
    }
  }
  if (a.ln_w != nullptr) {               // inner_attn_ln (dilated_attention.py:212-213): two-pass, biased variance
    const float mean = block_sum(part, red, tid) / (float)E;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxPairs; ++i)
      if (2 * tid + i * kStep < E) {
        const float d0 = val[i][0] - mean, d1 = val[i][1] - mean;
        q += d0 * d0 + d1 * d1;
      }
    const float rstd = rsqrtf(block_sum(q, red, tid) / (float)E + a.eps);
#pragma unroll
    for (int i = 0; i < kMaxPairs; ++i) {
      const int e = 2 * tid + i * kStep;
      if (e < E) {
        val[i][0] = (val[i][0] - mean) * rstd * a.ln_w[e] + a.ln_b[e];
        val[i][1] = (val[i][1] - mean) * rstd * a.ln_w[e + 1] + a.ln_b[e + 1];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kMaxPairs; ++i) {
    const int e = 2 * tid + i * kStep;
    if (e < E)
      *reinterpret_cast<uint32_t*>(a.out + (int64_t)slide * E + e) = pack2e<kH>(val[i][0], val[i][1]);
  }
}

// fills the geometry of `a`; returns the records per slide, or -1 on a bad schedule
int64_t cls_plan(ClsArgs& a, int64_t max_len, int H, const int32_t* seg_len, const int32_t* ratios, int nbranch) {
  int64_t items = 0;
  for (int b = 0; b < nbranch; ++b) {
    if (seg_len[b] < 1 || ratios[b] < 1) return -1;
    const GpBranch g = gp_make_branch(max_len, seg_len[b], ratios[b], H);
    a.sl[b] = seg_len[b];
    a.r[b] = ratios[b];
    a.hpg[b] = std::min(g.hpg, H);
    a.mc[b] = (g.m + kChunk - 1) / kChunk;
    a.pre[b] = (int32_t)items;
    items += (int64_t)a.hpg[b] * a.mc[b];
    if (items > 0x3fffffff) return -1;
  }
  a.pre[nbranch] = (int32_t)items;
  a.items = (int32_t)items;
  return items;
}

bool cls_shape_ok(int64_t max_len, int64_t nslide, int H, int D, int nbranch) {
  return max_len >= 1 && nslide >= 1 && nslide <= 65535 && H >= 1 && (D == 48 || D == 64 || D == 96) &&
         (int64_t)H * D <= 1536 && nbranch >= 1 && nbranch <= GP_MAX_BRANCHES;
}

template <int D>
void launch_partial(const ClsArgs& a, int fmt, dim3 grid, hipStream_t s) {
  if (fmt == GP_FMT_BF16) cls_attn_partial_kernel<D, false, false><<<grid, kChunk, 0, s>>>(a);
  else if (fmt == GP_FMT_F16) cls_attn_partial_kernel<D, true, true><<<grid, kChunk, 0, s>>>(a);
  else cls_attn_partial_kernel<D, true, false><<<grid, kChunk, 0, s>>>(a);
}

}  // namespace

extern "C" int64_t gp_cls_attn_workspace_bytes(int64_t max_len, int64_t nslide, int H, int D, const int32_t* seg_len,
                                               const int32_t* ratios, int nbranch) {
  if (!cls_shape_ok(max_len, nslide, H, D, nbranch) || !seg_len || !ratios) return -1;
  ClsArgs a = {};
  const int64_t items = cls_plan(a, max_len, H, seg_len, ratios, nbranch);
  return items < 0 ? -1 : nslide * items * (D + kRecHead) * (int64_t)sizeof(float);
}

extern "C" int gp_cls_attn_merge_ln(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t row_stride,
                                    const int64_t* slide_off, const int64_t* slide_len, int64_t nslide,
                                    int64_t max_len, int H, int D, const int32_t* seg_len, const int32_t* ratios,
                                    int nbranch, float softmax_scale, int q_log2_prescaled, int fmt,
                                    const float* ln_w, const float* ln_b, float eps, uint16_t* out, void* ws,
                                    int64_t ws_bytes, void* stream) {
  return gp_cls_attn_merge_ln_map(q, k, v, row_stride, slide_off, slide_len, nslide, max_len, nullptr, 0, H, D,
                                  seg_len, ratios, nbranch, softmax_scale, q_log2_prescaled, fmt, ln_w, ln_b, eps,
                                  out, ws, ws_bytes, stream);
}

extern "C" int gp_cls_attn_merge_ln_map(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t row_stride,
                                        const int64_t* slide_off, const int64_t* slide_len, int64_t nslide,
                                        int64_t max_len, const int32_t* row_map, int64_t map_rows, int H, int D,
                                        const int32_t* seg_len, const int32_t* ratios, int nbranch,
                                        float softmax_scale, int q_log2_prescaled, int fmt, const float* ln_w,
                                        const float* ln_b, float eps, uint16_t* out, void* ws, int64_t ws_bytes,
                                        void* stream) {
  gp_clear_error();
  GP_REQUIRE(row_map == nullptr || (map_rows >= 1 && map_rows <= max_len),
             "gp_cls_attn_merge_ln: a row map needs 1 <= map_rows (%lld) <= max_len", (long long)map_rows);
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16 || fmt == GP_FMT_F16_VBF16, "gp_cls_attn_merge_ln: bad fmt %d", fmt);
  GP_REQUIRE(cls_shape_ok(max_len, nslide, H, D, nbranch),
             "gp_cls_attn_merge_ln: bad shape (max_len %lld, nslide %lld, H %d, D %d in {48, 64, 96}, H*D <= 1536, "
             "nbranch %d)", (long long)max_len, (long long)nslide, H, D, nbranch);
  GP_REQUIRE(q && k && v && slide_off && slide_len && seg_len && ratios && out && ws,
             "gp_cls_attn_merge_ln: null pointer");
  GP_REQUIRE((ln_w == nullptr) == (ln_b == nullptr), "gp_cls_attn_merge_ln: ln_w and ln_b go together");
  GP_REQUIRE(row_stride >= (int64_t)H * D && row_stride % 8 == 0 && gp_aligned(q, 16) && gp_aligned(k, 16) &&
                 gp_aligned(v, 16) && gp_aligned(out, 4) && gp_aligned(ws, 16),
             "gp_cls_attn_merge_ln: q / k / v rows must be 16-byte aligned (row_stride %% 8 == 0)");
  ClsArgs a = {};
  const int64_t items = cls_plan(a, max_len, H, seg_len, ratios, nbranch);
  GP_REQUIRE(items > 0, "gp_cls_attn_merge_ln: bad segment schedule");
  const int64_t need = nslide * items * (D + kRecHead) * (int64_t)sizeof(float);
  GP_REQUIRE(ws_bytes >= need, "gp_cls_attn_merge_ln: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
             (long long)need);
  a.q = q; a.k = k; a.v = v;
  a.row_stride = row_stride;
  a.slide_off = slide_off;
  a.slide_len = slide_len;
  a.max_len = max_len;
  a.H = H; a.D = D; a.nbranch = nbranch;
  a.qk_scale = q_log2_prescaled ? 1.0f
                                : (softmax_scale > 0.f ? softmax_scale : 1.0f / sqrtf((float)D)) * 1.4426950408889634f;
  a.ln_w = ln_w; a.ln_b = ln_b; a.eps = eps;
  a.out = out;
  a.ws = static_cast<float*>(ws);
  a.row_map = row_map;
  a.map_rows = (int32_t)map_rows;
  hipStream_t s = gp_stream(stream);
  const dim3 grid((unsigned)items, (unsigned)nslide);
  if (D == 48) launch_partial<48>(a, fmt, grid, s);
  else if (D == 64) launch_partial<64>(a, fmt, grid, s);
  else launch_partial<96>(a, fmt, grid, s);
  if (int rc = gp_check_launch("gp_cls_attn_merge_ln (partial)")) return rc;
  const size_t lds = ((size_t)nbranch * H * D + (size_t)nbranch * H + kMergeWaves) * sizeof(float);
  if (fmt == GP_FMT_BF16) cls_merge_ln_kernel<false><<<(unsigned)nslide, 64 * kMergeWaves, lds, s>>>(a);
  else cls_merge_ln_kernel<true><<<(unsigned)nslide, 64 * kMergeWaves, lds, s>>>(a);
  return gp_check_launch("gp_cls_attn_merge_ln (merge)");
}
