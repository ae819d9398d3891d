// Opt-in second backward of the fused dilated attention for gfx950 (gp_dilated_attn_bwd2): the contract, the
// workspace and the launch sequence of gp_dilated_attn_bwd (gp_attn_bwd.hip) for the product arch's training case --
// D = 48, q pre-scaled by D^-0.5 log2 e, bf16 or fp16 -- with the forward's kernel design turned to the backward
// (DESIGN §3.18):
//   * a work item is (segment, head, 256 own rows) of one branch on 8 waves x 32 rows; the own rows' Q / dO (dQ
//     kernel) or K / V (dK/dV kernel) fragments live in registers;
//   * every product is a v_mfma_f32_32x32x16: S^T / dP^T contract d = 48 in three exact 16-deep steps, and their C
//     layout (a lane owns 16 tile rows of ONE own row) is the B operand of the gradient products as it stands, as P
//     is in the forward.  The gradient products write d as two 32-row blocks; rows 48..63 of the second repeat rows
//     32..47 (the transposed read of that block's upper half is aimed at the lower half) and are never stored;
//   * the streamed operand (K | V, or Q | dO) arrives in 64-row tiles by LDS-DMA into two 112-byte-row images, double
//     buffered, one barrier per tile; the per-tile buffer descriptors end at the last valid row, so tail rows read
//     as zeros with no predicated load, and the dilated gather is the per-row stride r * row_stride;
//   * both images serve row-wise ds_read_b128 fragments and ds_read_tr16_b64 transposed reads.
// Store-and-own, two launches per branch, no atomics, no inter-workgroup waits: two calls give the same bits.  The
// precision machinery of the first backward is kept: delta from the MFMA sequence of dP, the fp32 row sum eps of dS
// (summed on the VALU: the spare d rows stay idle), the pk correction of dq, the rounded dS plus its rounded
// remainder, and the corrected delta handed to the dK/dV kernel.  Compiled with NaNs honoured and without the packed
// fp32 VALU forms.  The merge backward, the geometry decode, the workspace layout and the final store are copies of
// gp_attn_bwd.hip's (that unit's object stays byte-identical).
#include <math.h>

#include "gp_api.h"
#include "gp_common.h"

namespace {

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) void lds_void;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int D = 48;
constexpr int NW = 8;                          // waves of a workgroup, 32 own rows each
constexpr int NT = NW * 64;
constexpr int kOwn = NW * 32;                  // 256 own rows (queries or keys)
constexpr int kTile = 64;                      // rows of a streamed tile
constexpr int ROWB = 2 * D + 16;               // 112-byte image rows: 7 sixteen-byte units, the last one padding
constexpr int UPR = ROWB / 16;                 // units per row
constexpr int CH = D / 8;                      // data units per row
constexpr int IMG = kTile * ROWB;              // 7168 bytes = 7 DMA pieces of 1 KiB
constexpr int PPI = IMG / 1024;                // pieces per image
constexpr int PPW = (2 * PPI + NW - 1) / NW;   // pieces per wave and tile (two images)
constexpr int BUF = 2 * IMG;
constexpr int STATB = 2 * kTile * 4;           // lse * log2(e) | delta of a query tile
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
static_assert(IMG % 1024 == 0, "an image is a whole number of 1 KiB DMA pieces");

template <bool kH>
GP_DEV f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {   // 32x32 += [32 x 16].[16 x 32]
  if constexpr (kH)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <bool kH>
GP_DEV __bf16 f2e_slot(float f) { return __builtin_bit_cast(__bf16, f2e<kH>(f)); }
GP_DEV f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// Blocks b, b + 8, ... share an XCD: give each XCD runs of 8 consecutive work items (as gp_attn.hip's xcd_group).
GP_DEV int64_t xcd_group(int64_t bid, int64_t nb) {
  constexpr int64_t G = 8, C = 8 * G;
  const int64_t full = nb - nb % C;
  if (bid >= full) return bid;
  const int64_t base = bid - bid % C;
  const int64_t in = bid % C;
  return base + (in & 7) * G + (in >> 3);
}

// One branch: dense q / k / v rows, the branch's own o / dout / lse / delta buffers (gp_attn_bwd.hip's DilArgs).
struct Args {
  const uint16_t *q, *k, *v;     // [B*L, row_stride], head h at columns h*D
  const uint16_t *o, *dout;      // [B*nseg, m, H, D]: the forward's o_b; w_b * dmerged (merge_bwd_kernel)
  const float* lse;              // [B*nseg, H, m]
  float* delta;                  // [B*nseg, H, m] fp32 (workspace)
  float *gq, *gk, *gv;           // fp32 accumulators [B*L, H*D]
  int64_t row_stride, L;
  GpBranch g;
  int32_t H;
  int32_t ntile;                 // ceil(m / kOwn)
};

// What one (segment, head) addresses: gp_attn_bwd.hip's View and dil_view.
struct View {
  const uint16_t *q, *k, *v, *dout, *o;
  const float* lse;
  float* delta;
  float *gq, *gk, *gv;
  int64_t rs, rso, grs;          // row strides of q / k / v, of o / dout, of the accumulators
  int nk, nq;                    // valid keys (= rows with a real q); query rows that carry a dout
  int npad;                      // zero-pad keys in the saved LSE (score 0, v = 0): m - nk
};
GP_DEV int make_view(const Args& a, int64_t item, View& w) {
  const GpBranch& g = a.g;
  const int tile = (int)(item % a.ntile);
  const int64_t bh = item / a.ntile;
  const int bn = (int)(bh / a.H), h = (int)(bh % a.H);
  const int bidx = bn / g.nseg, n = bn % g.nseg;
  const int64_t seg0 = (int64_t)bidx * g.nseg;
  const int j = h / g.hpg;
  const int64_t tok0 = (int64_t)bidx * a.L + (int64_t)n * g.s + j;       // the token of sparse row 0
  const int64_t off = tok0 * a.row_stride + h * D;
  w.q = a.q + off; w.k = a.k + off; w.v = a.v + off;
  const int64_t ooff = (seg0 * g.m + (int64_t)n * g.m) * a.H * D + h * D;
  w.dout = a.dout + ooff;
  w.o = a.o + ooff;
  const int64_t soff = ((seg0 + n) * a.H + h) * g.m;
  w.lse = a.lse + soff;
  w.delta = a.delta + soff;
  const int64_t goff = tok0 * ((int64_t)a.H * D) + h * D;
  w.gq = a.gq + goff; w.gk = a.gk + goff; w.gv = a.gv + goff;
  w.rs = a.row_stride * g.r;
  w.rso = (int64_t)a.H * D;
  w.grs = (int64_t)a.H * D * g.r;
  w.nk = gp_valid_rows(g, a.L, n, j);
  const int64_t lim = a.L - ((int64_t)n * g.g + j);                      // merge slots n g + i r + j < L
  const int64_t nq = lim > 0 ? (lim + g.r - 1) / g.r : 0;
  w.nq = (int)(nq < g.m ? nq : g.m);
  w.npad = g.m - w.nk;
  return tile;
}

GP_DEV void add_f32x4(float* p, float a, float b, float c, float d, float f) {   // read-add-write, 16-byte aligned
  f32x4* q = reinterpret_cast<f32x4*>(p);
  f32x4 x = *q;
  x[0] += a * f; x[1] += b * f; x[2] += c * f; x[3] += d * f;
  *q = x;
}

// The three k-steps of an own row as MFMA operands: lane (l32, hh) holds d = 16 ks + 8 hh .. + 7 of row l32.
struct Frag { bf16x8 f[3]; };
GP_DEV void load_frag(Frag& r, const uint16_t* row, int hh, bool valid) {
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) {
    bf16x8 z = {};
    if (valid) z = *reinterpret_cast<const bf16x8*>(row + 16 * ks + 8 * hh);
    r.f[ks] = z;
  }
}
// acc[tile row][own row] of a 32-row sub-tile: the image's rows (row-wise ds_read_b128) against an own-row fragment
template <bool kH>
GP_DEV f32x16 dot_tile(const char* img, int row, int hh, const Frag& b) {
  f32x16 acc = zero16();
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(img + row * ROWB + 32 * ks + 16 * hh);
    acc = mfma<kH>(a, b.f[ks], acc);
  }
  return acc;
}
// A operand X^T[d 32 mt + l32][tile row] of a product that contracts over 16 tile rows, by two transposed reads of
// X's row-major image: element e < 4 is tile row r16 + 4 hh + e, e >= 4 is r16 + 8 + 4 hh + e - 4 -- the rows that
// registers 8 s .. 8 s + 7 of a 32x32 C tile hold.  The 16-lane group (hh, c) reads four rows x 16 d of block
// 2 mt + c; block 3 (d 48..63) does not exist and is aimed at block 2.
GP_DEV bf16x8 read_transposed(const char* img, int r16, int mt, int lane) {
  const int hh = lane >> 5, c = (lane >> 4) & 1;
  const int blk = mt ? 2 : c;
  const char* p0 = img + (r16 + 4 * hh + ((lane >> 2) & 3)) * ROWB + 32 * blk + 8 * (lane & 3);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0 + 8 * ROWB));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// LDS-DMA of two [kTile x D] images per tile.  Piece pc of the 14 goes to wave pc % NW: 64 lane-linear 16-byte
// units of image pc / 7; unit u is row u / 7, chunk u % 7, and the lanes of the padding chunk are off.
struct Dma {
  int voff[PPW];                 // byte offset of the lane's unit from its image's tile base
  unsigned mask;                 // bit sl: the lane's unit of slot sl is data
  GP_DEV void init(int w, int lane, int64_t rs0, int64_t rs1) {
    mask = 0;
#pragma unroll
    for (int sl = 0; sl < PPW; ++sl) {
      const int pc = w + NW * sl;
      voff[sl] = 0;
      if (pc >= 2 * PPI) continue;
      const int unit = (pc % PPI) * 64 + lane, row = unit / UPR, ch = unit % UPR;
      voff[sl] = (int)((int64_t)row * (pc < PPI ? rs0 : rs1) * 2 + (ch < CH ? ch : 0) * 16);
      if (ch < CH) mask |= 1u << sl;
    }
  }
  // x0 / x1: row row0 of the two operands; n0 / n1: their valid rows from row0 on (> 0 for one of them)
  GP_DEV void load(char* buf, int w, const uint16_t* x0, int64_t rs0, int n0, const uint16_t* x1, int64_t rs1,
                   int n1) const {
    const int r0 = n0 < kTile ? n0 : kTile, r1 = n1 < kTile ? n1 : kTile;
    const int rec0 = r0 > 0 ? (int)((r0 - 1) * rs0 * 2 + 2 * D) : 0;
    const int rec1 = r1 > 0 ? (int)((r1 - 1) * rs1 * 2 + 2 * D) : 0;
    const __amdgpu_buffer_rsrc_t d0 = __builtin_amdgcn_make_buffer_rsrc((void*)x0, (short)0, rec0, 0x00020000);
    const __amdgpu_buffer_rsrc_t d1 = __builtin_amdgcn_make_buffer_rsrc((void*)x1, (short)0, rec1, 0x00020000);
#pragma unroll
    for (int sl = 0; sl < PPW; ++sl) {
      const int pc = w + NW * sl;
      if (pc < 2 * PPI && ((mask >> sl) & 1u))
        __builtin_amdgcn_raw_ptr_buffer_load_lds(pc < PPI ? d0 : d1, (lds_void*)(buf + pc * 1024), 16, voff[sl], 0, 0, 0);
    }
  }
};
GP_DEV void dma_wait_and_sync() {
  __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): this wave's DMA pieces landed
  __syncthreads();
}

// ---------------------------------------------------------------------------------------
// dQ (and the corrected delta): one workgroup per 256 query rows of a (segment, head); K | V streamed.
template <bool kH>
__global__ __launch_bounds__(NT) void attn_bwd2_dq_kernel(const Args a) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * BUF];   // [K0 | V0 | K1 | V1]

  const int64_t item = xcd_group(blockIdx.x, gridDim.x);
  View vw;
  const int tile = make_view(a, item, vw);
  const int nk = vw.nk;
  const int nst = vw.nk < vw.nq ? vw.nk : vw.nq;     // rows whose dq is stored
  if (tile * kOwn >= vw.nq || nk == 0) return;       // no row with a dout here
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  const int l32 = lane & 31, hh = lane >> 5;
  const int64_t rs = vw.rs;
  const int i = tile * kOwn + w * 32 + l32;          // the lane's query row
  const bool valid = i < vw.nq;                      // carries a dout (a zero-pad query past nk: q = 0)
  const bool wact = __builtin_amdgcn_readfirstlane(tile * kOwn + w * 32) < vw.nq;

  Dma dma;
  dma.init(w, lane, rs, rs);
  dma.load(smem, w, vw.k, rs, nk, vw.v, rs, nk);

  // Q / dO fragments (B operands: column = query l32), delta and lse of the lane's row
  Frag qf, dof, of;
  load_frag(qf, vw.q + (int64_t)i * rs, hh, i < nk);
  load_frag(dof, vw.dout + (int64_t)i * vw.rso, hh, valid);
  load_frag(of, vw.o + (int64_t)i * vw.rso, hh, valid);
  // delta: the diagonal of O.dO^T, summed exactly as dP sums V.dO^T.  Row n of column n is register
  // (n & 3) + 4 (n >> 3) of the lane (n, (n >> 2) & 1).
  float dl;
  {
    f32x16 dd = zero16();
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) dd = mfma<kH>(of.f[ks], dof.f[ks], dd);
    const int want = (l32 & 3) + 4 * (l32 >> 3);
    float pick = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) pick = r == want ? dd[r] : pick;
    dl = __shfl(pick, l32 + 32 * ((l32 >> 2) & 1), 64);
  }
  const float lse2 = valid ? vw.lse[i] * kLog2e : INFINITY;

  // acc: dQ^T[d 32 mt + ..][q]; pk: sum_j P_ij k_j, the first-order correction of dq for the error eps of delta
  // (gp_attn_bwd.hip, attn_bwd_dq_kernel)
  f32x16 acc[2], pk[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) { acc[mt] = zero16(); pk[mt] = zero16(); }
  float eps = 0.f;

  const int ntiles = (nk + kTile - 1) / kTile;
  dma_wait_and_sync();
  for (int t = 0; t < ntiles; ++t) {
    const int kv0 = t * kTile;
    if (t + 1 < ntiles)
      dma.load(smem + ((t + 1) & 1) * BUF, w, vw.k + (int64_t)(kv0 + kTile) * rs, rs, nk - kv0 - kTile,
               vw.v + (int64_t)(kv0 + kTile) * rs, rs, nk - kv0 - kTile);
    const char* Kb = smem + (t & 1) * BUF;
    const char* Vb = Kb + IMG;
    const bool tail = kv0 + kTile > nk;
    if (wact) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        // S^T / dP^T [key][q]: the lane holds keys 32 u + (r & 3) + 8 (r >> 2) + 4 hh of query l32
        const f32x16 sacc = dot_tile<kH>(Kb, 32 * u + l32, hh, qf);
        const f32x16 dpacc = dot_tile<kH>(Vb, 32 * u + l32, hh, dof);
        bf16x8 dsf[2], dsl[2], pf[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float p = __builtin_amdgcn_exp2f(sacc[r] - lse2);
          if (tail) p = (kv0 + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * hh < nk) ? p : 0.f;
          const float ds = p * (dpacc[r] - dl);
          const uint16_t dsb = f2e<kH>(ds);
          eps += ds;
          dsf[r >> 3][r & 7] = __builtin_bit_cast(__bf16, dsb);
          dsl[r >> 3][r & 7] = f2e_slot<kH>(ds - e2f<kH>(dsb));   // what the rounding of dS dropped
          pf[r >> 3][r & 7] = f2e_slot<kH>(p);
        }
        // dQ^T[d][q] += K^T[d][key] . dS^T[key][q];  pk^T[d][q] += K^T[d][key] . P^T[key][q]
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) {
            const bf16x8 kT = read_transposed(Kb, 32 * u + 16 * s, mt, lane);
            acc[mt] = mfma<kH>(kT, dsf[s], acc[mt]);
            acc[mt] = mfma<kH>(kT, dsl[s], acc[mt]);
            pk[mt] = mfma<kH>(kT, pf[s], pk[mt]);
          }
      }
    }
    dma_wait_and_sync();
  }
  if (!wact) return;

  // the two lanes of a query hold its keys 4 hh + ..; the zero pads add P (0 - delta)
  eps += __shfl_xor(eps, 32, 64);
  eps -= (float)vw.npad * __builtin_amdgcn_exp2f(-lse2) * dl;
  if (valid && hh == 0) vw.delta[i] = dl + eps;
  if (i < nst) {
    float* row = vw.gq + (int64_t)i * vw.grs;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int rg = 0; rg < (mt ? 2 : 4); ++rg) {
        float x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = acc[mt][4 * rg + e] - pk[mt][4 * rg + e] * eps;
        add_f32x4(row + 32 * mt + 8 * rg + 4 * hh, x[0], x[1], x[2], x[3], kLn2);
      }
  }
}

// ---------------------------------------------------------------------------------------
// dK / dV: one workgroup per 256 keys of a (segment, head); Q | dO + lse | delta streamed.
template <bool kH>
__global__ __launch_bounds__(NT) void attn_bwd2_dkv_kernel(const Args a) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * BUF + 2 * STATB];   // [Q0 | dO0 | Q1 | dO1 | stat0 | stat1]

  const int64_t item = xcd_group(blockIdx.x, gridDim.x);
  View vw;
  const int tile = make_view(a, item, vw);
  const int nq = vw.nq;                              // query rows that carry a dout
  const int nkey = vw.nk;
  if (tile * kOwn >= nkey || nq == 0) return;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  const int l32 = lane & 31, hh = lane >> 5;
  const int64_t rs = vw.rs, rso = vw.rso;
  const int key = tile * kOwn + w * 32 + l32;        // the lane's key
  const bool wact = __builtin_amdgcn_readfirstlane(tile * kOwn + w * 32) < nkey;

  Dma dma;
  dma.init(w, lane, rs, rso);
  dma.load(smem, w, vw.q, rs, nkey, vw.dout, rso, nq);     // a query row past nkey is a zero pad

  // threads 0..63: lse * log2(e) (+inf past nq: P = 0), 64..127: delta (0 past nq) of tile row tid & 63
  float sv = 0.f;
  auto load_stat = [&](int row0) {
    if (threadIdx.x < 2 * kTile) {
      const int qi = row0 + ((int)threadIdx.x & (kTile - 1));
      if (threadIdx.x < kTile) sv = qi < nq ? vw.lse[qi] * kLog2e : INFINITY;
      else sv = qi < nq ? vw.delta[qi] : 0.f;
    }
  };
  auto store_stat = [&](int buf) {
    if (threadIdx.x < 2 * kTile) reinterpret_cast<float*>(smem + 2 * BUF + buf * STATB)[threadIdx.x] = sv;
  };
  load_stat(0);
  store_stat(0);

  // K / V fragments (B operands: column = key l32)
  Frag kf, vf;
  load_frag(kf, vw.k + (int64_t)key * rs, hh, key < nkey);
  load_frag(vf, vw.v + (int64_t)key * rs, hh, key < nkey);

  f32x16 dkacc[2], dvacc[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) { dkacc[mt] = zero16(); dvacc[mt] = zero16(); }

  const int ntiles = (nq + kTile - 1) / kTile;
  dma_wait_and_sync();
  for (int t = 0; t < ntiles; ++t) {
    const int q1 = (t + 1) * kTile;
    if (t + 1 < ntiles) {
      dma.load(smem + ((t + 1) & 1) * BUF, w, vw.q + (int64_t)q1 * rs, rs, nkey - q1, vw.dout + (int64_t)q1 * rso, rso,
               nq - q1);
      load_stat(q1);
    }
    const char* Qb = smem + (t & 1) * BUF;
    const char* Ob = Qb + IMG;
    const float* stat = reinterpret_cast<const float*>(smem + 2 * BUF + (t & 1) * STATB);
    if (wact) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        // S / dP [q][key]: the lane holds queries 32 u + (r & 3) + 8 (r >> 2) + 4 hh of key l32
        const f32x16 sacc = dot_tile<kH>(Qb, 32 * u + l32, hh, kf);
        const f32x16 dpacc = dot_tile<kH>(Ob, 32 * u + l32, hh, vf);
        bf16x8 pf[2], dsf[2];
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(stat + 32 * u + 8 * rg + 4 * hh);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(stat + kTile + 32 * u + 8 * rg + 4 * hh);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * rg + e;
            const float p = __builtin_amdgcn_exp2f(sacc[r] - l4[e]);   // tail query: exp2(-inf) = 0
            pf[r >> 3][r & 7] = f2e_slot<kH>(p);
            dsf[r >> 3][r & 7] = f2e_slot<kH>(p * (dpacc[r] - d4[e]));
          }
        }
        // dV^T[d][key] += dO^T[d][q] . P[q][key];  dK^T[d][key] += Q^T[d][q] . dS[q][key]
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) {
            const bf16x8 oT = read_transposed(Ob, 32 * u + 16 * s, mt, lane);
            const bf16x8 qT = read_transposed(Qb, 32 * u + 16 * s, mt, lane);
            dvacc[mt] = mfma<kH>(oT, pf[s], dvacc[mt]);
            dkacc[mt] = mfma<kH>(qT, dsf[s], dkacc[mt]);
          }
      }
    }
    if (t + 1 < ntiles) store_stat((t + 1) & 1);
    dma_wait_and_sync();
  }

  if (wact && key < nkey) {
    const int64_t off = (int64_t)key * vw.grs;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int rg = 0; rg < (mt ? 2 : 4); ++rg) {
        const int d0 = 32 * mt + 8 * rg + 4 * hh, r = 4 * rg;
        add_f32x4(vw.gk + off + d0, dkacc[mt][r], dkacc[mt][r + 1], dkacc[mt][r + 2], dkacc[mt][r + 3], kLn2);
        add_f32x4(vw.gv + off + d0, dvacc[mt][r], dvacc[mt][r + 1], dvacc[mt][r + 2], dvacc[mt][r + 3], 1.f);
      }
  }
}

// ---------------------------------------------------------------------------------------
// Backward of the merge without its LayerNorm, one thread per (token, head): gp_attn_bwd.hip's merge_bwd_kernel.
// The branch weights (uncovered or lse == 0 -> -1e8, fp32 softmax over the branches) take no gradient; the sparse
// row whose merge slot is the token receives dout_b = w_b dmerged, rounded to the format.
struct MergeBwdArgs {
  const float* lse[GP_MAX_BRANCHES];
  uint16_t* dout[GP_MAX_BRANCHES];
  GpBranch g[GP_MAX_BRANCHES];
  const uint16_t* dmerged;
  int64_t B, L;
  int32_t H, nbranch;
};

template <bool kH>
__global__ __launch_bounds__(256) void merge_bwd2_kernel(const MergeBwdArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.B * a.L * a.H) return;
  const int h = (int)(idx % a.H);
  const int64_t tok = idx / a.H;
  const int bidx = (int)(tok / a.L), p = (int)(tok % a.L);
  const uint16_t* dm = a.dmerged + (tok * a.H + h) * D;
  float e[GP_MAX_BRANCHES];
  uint16_t* drows[GP_MAX_BRANCHES];
  bool cov[GP_MAX_BRANCHES];
  float mx = -INFINITY;
#pragma unroll
  for (int b = 0; b < GP_MAX_BRANCHES; ++b) {
    e[b] = -1e8f; cov[b] = false; drows[b] = nullptr;
    if (b < a.nbranch) {
      const GpBranch g = a.g[b];
      const int64_t seg0 = (int64_t)bidx * g.nseg;
      const int n = p / g.g, pt = p - n * g.g;
      const int i = pt / g.r, j = pt - i * g.r;
      cov[b] = h / g.hpg == j;
      drows[b] = a.dout[b] + (((seg0 + n) * g.m + i) * a.H + h) * D;
      if (cov[b]) e[b] = a.lse[b][((seg0 + n) * a.H + h) * g.m + i];
      if (!cov[b] || e[b] == 0.f) e[b] = -1e8f;
      mx = fmaxf(mx, e[b]);
    }
  }
  float wsum = 0.f;
#pragma unroll
  for (int b = 0; b < GP_MAX_BRANCHES; ++b)
    if (b < a.nbranch) {
      e[b] = __builtin_amdgcn_exp2f((e[b] - mx) * kLog2e);
      wsum += e[b];
    }
  const float inv = __builtin_amdgcn_rcpf(wsum);
#pragma unroll
  for (int b = 0; b < GP_MAX_BRANCHES; ++b)
    if (b < a.nbranch && cov[b]) {
      const float wb = e[b] * inv;
#pragma unroll
      for (int c = 0; c < D; c += 8) {
        float x[8];
        load_e<kH, 8>(dm + c, x);
        *reinterpret_cast<uint4*>(drows[b] + c) = make_uint4(pack2e<kH>(x[0] * wb, x[1] * wb), pack2e<kH>(x[2] * wb, x[3] * wb),
                                                             pack2e<kH>(x[4] * wb, x[5] * wb), pack2e<kH>(x[6] * wb, x[7] * wb));
      }
    }
}

// The one rounding of the accumulated gradients: fp32 [rows, E] planes -> dq / dk / dv rows (stride ds).
template <bool kH>
__global__ __launch_bounds__(256) void grad_store2_kernel(const float* gq, const float* gk, const float* gv, uint16_t* dq,
                                                          uint16_t* dk, uint16_t* dv, int64_t ds, int64_t rows, int E) {
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

// gp_dilated_attn_bwd's workspace layout: per branch dout_b (16-bit) and delta_b (fp32), then three fp32 accumulators
struct Ws {
  size_t dout[GP_MAX_BRANCHES], delta[GP_MAX_BRANCHES], g[3], total;
  GpBranch geo[GP_MAX_BRANCHES];
};
bool ws_layout(int64_t B, int64_t L, int H, int Dh, const int32_t* seg_len, const int32_t* ratios, int nbranch, Ws& w) {
  if (B <= 0 || L <= 0 || H <= 0 || H > 4096 || Dh != D || !seg_len || !ratios || nbranch < 1 || nbranch > GP_MAX_BRANCHES)
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

template <bool kH>
void launch(const MergeBwdArgs& m, Args a, const Ws& w, char* ws, const uint16_t* const* o_in, int64_t B, uint16_t* dq,
            uint16_t* dk, uint16_t* dv, int64_t ds, hipStream_t s) {
  const int64_t th = B * m.L * m.H;
  merge_bwd2_kernel<kH><<<(unsigned)((th + 255) / 256), 256, 0, s>>>(m);
  for (int b = 0; b < m.nbranch; ++b) {                    // fixed order: each branch adds into the accumulators
    a.g = w.geo[b];
    a.o = o_in[b];
    a.dout = m.dout[b];
    a.lse = m.lse[b];
    a.delta = reinterpret_cast<float*>(ws + w.delta[b]);
    a.ntile = (a.g.m + kOwn - 1) / kOwn;
    const unsigned grid = (unsigned)(B * a.g.nseg * m.H * a.ntile);
    attn_bwd2_dq_kernel<kH><<<grid, NT, 0, s>>>(a);
    attn_bwd2_dkv_kernel<kH><<<grid, NT, 0, s>>>(a);
  }
  const int E = m.H * D;
  const int64_t n4 = B * m.L * (E / 4);
  grad_store2_kernel<kH><<<(unsigned)((n4 + 255) / 256), 256, 0, s>>>(a.gq, a.gk, a.gv, dq, dk, dv, ds, B * m.L, E);
}

}  // namespace

extern "C" size_t gp_dilated_attn_bwd2_workspace_bytes(int64_t B, int64_t L, int H, int Dh, const int32_t* seg_len,
                                                       const int32_t* ratios, int nbranch) {
  Ws w;
  return ws_layout(B, L, H, Dh, seg_len, ratios, nbranch, w) ? w.total : 0;
}

extern "C" int gp_dilated_attn_bwd2(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t row_stride,
                                    int64_t B, int64_t L, int H, int Dh, const int32_t* seg_len, const int32_t* ratios,
                                    int nbranch, const uint16_t* const* o_in, const float* const* lse_in,
                                    const uint16_t* dmerged, float softmax_scale, int q_log2_prescaled, uint16_t* dq,
                                    uint16_t* dk, uint16_t* dv, int64_t d_row_stride, void* workspace,
                                    size_t workspace_bytes, int fmt, void* stream) {
  (void)softmax_scale;               // the logit is q'.k in the log2 domain: dq' = ln 2 dS k, dk = ln 2 dS^T q'
  GP_REQUIRE(Dh == D, "gp_dilated_attn_bwd2: head dim D = %d unsupported (D = 48 only)", Dh);
  GP_REQUIRE(q_log2_prescaled, "gp_dilated_attn_bwd2: q_log2_prescaled must be 1 (q pre-scaled by D^-0.5 log2 e)");
  GP_REQUIRE(fmt == GP_FMT_BF16 || fmt == GP_FMT_F16, "gp_dilated_attn_bwd2: bad fmt %d (GP_FMT_BF16 or GP_FMT_F16)", fmt);
  GP_REQUIRE(nbranch >= 1 && nbranch <= GP_MAX_BRANCHES, "gp_dilated_attn_bwd2: nbranch must be 1..%d (got %d)",
             GP_MAX_BRANCHES, nbranch);
  GP_REQUIRE(B > 0 && L > 0 && H > 0 && H <= 4096 && B <= (int64_t)0x7fffffff / L,
             "gp_dilated_attn_bwd2: bad sizes B %lld, L %lld, H %d", (long long)B, (long long)L, H);
  const void* ptrs[] = {q, k, v, dmerged, dq, dk, dv};
  const char* names[] = {"q", "k", "v", "dmerged", "dq", "dk", "dv"};
  for (int i = 0; i < 7; ++i) {
    GP_REQUIRE(ptrs[i] != nullptr, "gp_dilated_attn_bwd2: null pointer (%s)", names[i]);
    GP_REQUIRE(gp_aligned(ptrs[i], 16), "gp_dilated_attn_bwd2: misaligned pointer (%s)", names[i]);
  }
  GP_REQUIRE(seg_len && ratios && o_in && lse_in, "gp_dilated_attn_bwd2: null pointer (%s)",
             !seg_len ? "seg_len" : !ratios ? "ratios" : !o_in ? "o_in" : "lse_in");
  const int64_t E = (int64_t)H * D;
  GP_REQUIRE(row_stride >= E && row_stride % 8 == 0,
             "gp_dilated_attn_bwd2: row_stride %lld below H*D = %lld or not a multiple of 8", (long long)row_stride,
             (long long)E);
  GP_REQUIRE(d_row_stride >= E && d_row_stride % 8 == 0,
             "gp_dilated_attn_bwd2: d_row_stride %lld below H*D = %lld or not a multiple of 8", (long long)d_row_stride,
             (long long)E);
  for (int b = 0; b < nbranch; ++b) {
    GP_REQUIRE(seg_len[b] > 0 && ratios[b] > 0, "gp_dilated_attn_bwd2: branch %d: bad seg_len %d / ratio %d", b,
               seg_len[b], ratios[b]);
    // a tile's 64 gathered rows are addressed by 32-bit byte offsets from the tile's first row
    GP_REQUIRE(row_stride * ratios[b] * 2 * kTile < (int64_t)0x7fffffff,
               "gp_dilated_attn_bwd2: branch %d: row_stride %lld x ratio %d too large for a tile's 32-bit offsets", b,
               (long long)row_stride, ratios[b]);
    GP_REQUIRE(o_in[b] != nullptr && lse_in[b] != nullptr, "gp_dilated_attn_bwd2: null pointer (o_in / lse_in [%d])", b);
    GP_REQUIRE(gp_aligned(o_in[b], 16) && gp_aligned(lse_in[b], 4),
               "gp_dilated_attn_bwd2: misaligned pointer (o_in / lse_in [%d])", b);
  }
  Ws w;
  GP_REQUIRE(ws_layout(B, L, H, Dh, seg_len, ratios, nbranch, w), "gp_dilated_attn_bwd2: bad shape");
  GP_REQUIRE(workspace != nullptr && workspace_bytes >= w.total,
             "gp_dilated_attn_bwd2: workspace too small (%zu bytes, gp_dilated_attn_bwd2_workspace_bytes asks %zu)",
             workspace ? workspace_bytes : (size_t)0, w.total);
  GP_REQUIRE(gp_aligned(workspace, 16), "gp_dilated_attn_bwd2: misaligned workspace (16 bytes)");
  for (int b = 0; b < nbranch; ++b) {
    const int64_t items = B * w.geo[b].nseg * H * ((w.geo[b].m + kOwn - 1) / kOwn);
    GP_REQUIRE(items < (int64_t)0x7fffffff, "gp_dilated_attn_bwd2: branch %d: %lld work items exceed one launch", b,
               (long long)items);
  }
  GP_REQUIRE((B * L * H + 255) / 256 < (int64_t)0x7fffffff && (B * L * (E / 4) + 255) / 256 < (int64_t)0x7fffffff,
             "gp_dilated_attn_bwd2: B*L*H*D too large for one launch");

  char* ws = static_cast<char*>(workspace);
  MergeBwdArgs m = {};
  for (int b = 0; b < nbranch; ++b) {
    m.lse[b] = lse_in[b];
    m.dout[b] = reinterpret_cast<uint16_t*>(ws + w.dout[b]);
    m.g[b] = w.geo[b];
  }
  m.dmerged = dmerged;
  m.B = B; m.L = L; m.H = H; m.nbranch = nbranch;
  Args a = {};
  a.q = q; a.k = k; a.v = v;
  a.gq = reinterpret_cast<float*>(ws + w.g[0]);
  a.gk = reinterpret_cast<float*>(ws + w.g[1]);
  a.gv = reinterpret_cast<float*>(ws + w.g[2]);
  a.row_stride = row_stride; a.L = L; a.H = H;
  hipStream_t s = gp_stream(stream);
  // the accumulators start at zero: a (token, head) no branch covers keeps it
  const hipError_t me = hipMemsetAsync(ws + w.g[0], 0, w.total - w.g[0], s);
  if (me != hipSuccess) {
    gp_set_error("gp_dilated_attn_bwd2: hipMemsetAsync: %s", hipGetErrorString(me));
    return (int)me;
  }
  if (fmt == GP_FMT_F16) launch<true>(m, a, w, ws, o_in, B, dq, dk, dv, d_row_stride, s);
  else launch<false>(m, a, w, ws, o_in, B, dq, dk, dv, d_row_stride, s);
  return gp_check_launch("gp_dilated_attn_bwd2");
}
