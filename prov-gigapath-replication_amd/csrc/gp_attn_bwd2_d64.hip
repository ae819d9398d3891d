// Packed (varlen) attention backward at D = 64 for gfx950 (gp_dilated_attn_bwd2_varlen): the 32x32 MFMA, LDS-DMA design
// of gp_attn_bwd2.hip at the head dim where it fits without waste, over slides packed token-major in one
// qkv buffer.  bf16, q pre-scaled by D^-0.5 log2 e -- what the packed D = 64 forward takes.
//   * a work item is (slide, segment, head, 256 own rows) of one branch on 8 waves x 32 rows.  The slide is found by a
//     binary search of the branch's table of exclusive item prefixes on a value derived from blockIdx alone (after the
//     XCD grouping), so it is wave-uniform; its 64-byte entry comes by scalar loads and carries the slide's own L, from
//     which nk / nq / npad follow.  Nothing in the kernels knows T: the next slide's CLS row is a tail row like any other;
//   * every product is a v_mfma_f32_32x32x16_bf16: S^T / dP^T contract d = 64 in four exact 16-deep steps, and both
//     32-row d blocks of the gradient products hold data (no padded half block, no aliased transposed read);
//   * the streamed operand (K | V, or Q | dO) arrives in 64-row tiles by LDS-DMA into two 144-byte-row images (9
//     sixteen-byte units, the last one padding: odd, so row-wise ds_read_b128 is conflict-free), 9 one-KiB pieces per
//     image, 18 per tile over 8 waves (three slots per wave, the third used by waves 0 and 1), double buffered, one
//     barrier per tile.  The per-tile buffer descriptors end at the last valid row of the slide's segment: tail rows
//     read as zeros and no row of a neighbouring slide is read; the dilated gather is the row stride r * row_stride.
// Store-and-own, two launches per branch, no atomics, no inter-workgroup waits: two calls give the same bits.  The
// precision machinery is that of the first backward: delta from the MFMA sequence of dP, the fp32 row
// sum eps of dS (a VALU sum), the pk correction of dq, the rounded dS plus its rounded remainder, and the corrected
// delta handed to the dK/dV kernel.  Compiled with NaNs honoured and without the packed fp32 VALU forms.  The merge
// backward, the geometry decode, the table entry and the final store are copies of gp_attn_bwd.hip's (that unit's
// object stays byte-identical).
#include <math.h>
#include <string.h>

#include "gp_api.h"
#include "gp_common.h"

namespace {

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) void lds_void;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int D = 64;
constexpr int KS = D / 16;                     // 16-deep k-steps of a product that contracts d
constexpr int NW = 8;                          // waves of a workgroup, 32 own rows each
constexpr int NT = NW * 64;
constexpr int kOwn = NW * 32;                  // 256 own rows (queries or keys)
constexpr int kTile = 64;                      // rows of a streamed tile
constexpr int ROWB = 2 * D + 16;               // 144-byte image rows: 9 sixteen-byte units, the last one padding
constexpr int UPR = ROWB / 16;                 // units per row
constexpr int CH = D / 8;                      // data units per row
constexpr int IMG = kTile * ROWB;              // 9216 bytes = 9 DMA pieces of 1 KiB
constexpr int PPI = IMG / 1024;                // pieces per image
constexpr int PPW = (2 * PPI + NW - 1) / NW;   // pieces per wave and tile (two images): 3
constexpr int BUF = 2 * IMG;
constexpr int STATB = 2 * kTile * 4;           // lse * log2(e) | delta of a query tile
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
static_assert(IMG % 1024 == 0, "an image is a whole number of 1 KiB DMA pieces");
static_assert(UPR % 2 == 1, "an odd unit count per row keeps row-wise 16-byte reads conflict-free");

GP_DEV f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {   // 32x32 += [32 x 16].[16 x 32]
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
GP_DEV __bf16 f2bf_slot(float f) { return __builtin_bit_cast(__bf16, f2bf(f)); }
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

// One slide of one branch (device table, [nbranch][nslide]): gp_attn_bwd.hip's VarEntry with 256-row own blocks.
struct Entry {
  GpBranch g;                    // the branch's geometry for this slide's L
  int32_t ntile;                 // ceil(g.m / kOwn)
  int32_t item_begin;            // exclusive prefix of nseg * H * ntile over the branch's slides
  int64_t L;                     // the slide's length (CLS + tiles)
  int64_t tok0;                  // its first packed row
  int64_t o_off, lse_off;        // elements: its region in the branch's packed o / dout and lse / delta buffers
};
static_assert(sizeof(Entry) == 64, "Entry is read as 16 words");

// One branch: the packed q / k / v rows and the branch's packed buffers.
struct Args {
  const uint16_t *q, *k, *v;     // [T, row_stride], head h at columns h*D
  const uint16_t *o, *dout;      // slide-major regions [nseg_i, m_i, H, D]: the forward's o_b; w_b * dmerged
  const float* lse;              // slide-major regions [nseg_i, H, m_i]
  float* delta;                  // as lse, fp32 (workspace)
  float *gq, *gk, *gv;           // fp32 accumulators [T, H*D]
  int64_t row_stride;
  const Entry* tab;              // this branch's nslide entries
  int32_t nslide, H;
};

// What one (slide, segment, head) addresses: gp_attn_bwd.hip's View.
struct View {
  const uint16_t *q, *k, *v, *dout, *o;
  const float* lse;
  float* delta;
  float *gq, *gk, *gv;
  int64_t rs, rso, grs;          // row strides of q / k / v, of o / dout, of the accumulators
  int nk, nq;                    // valid keys (= rows with a real q); query rows that carry a dout
  int npad;                      // zero-pad keys in the saved LSE (score 0, v = 0): m - nk
};

// Segment n, head h of the slide of entry e (gp_attn_bwd.hip's dil_view).  Every row limit is taken against the
// slide's own length e.L.
GP_DEV void dil_view(const Args& a, const Entry& e, int n, int h, View& w) {
  const GpBranch& g = e.g;
  const int j = h / g.hpg;
  const int64_t tok0 = e.tok0 + (int64_t)n * g.s + j;                    // the packed row of sparse row 0
  const int64_t off = tok0 * a.row_stride + h * D;
  w.q = a.q + off; w.k = a.k + off; w.v = a.v + off;
  const int64_t ooff = e.o_off + ((int64_t)n * g.m * a.H + h) * D;
  w.dout = a.dout + ooff;
  w.o = a.o + ooff;
  const int64_t soff = e.lse_off + ((int64_t)n * a.H + h) * g.m;
  w.lse = a.lse + soff;
  w.delta = a.delta + soff;
  const int64_t goff = tok0 * ((int64_t)a.H * D) + h * D;
  w.gq = a.gq + goff; w.gk = a.gk + goff; w.gv = a.gv + goff;
  w.rs = a.row_stride * g.r;
  w.rso = (int64_t)a.H * D;
  w.grs = (int64_t)a.H * D * g.r;
  w.nk = gp_valid_rows(g, e.L, n, j);
  const int64_t lim = e.L - ((int64_t)n * g.g + j);                      // merge slots n g + i r + j < L
  const int64_t nq = lim > 0 ? (lim + g.r - 1) / g.r : 0;
  w.nq = (int)(nq < g.m ? nq : g.m);
  w.npad = g.m - w.nk;
}

// A table entry by scalar loads (wave-uniform address, constant address space) instead of flat loads into VGPRs.
GP_DEV void load_entry_scalar(const Entry* src_entry, Entry& e) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t words[sizeof(Entry) / 4];
  const __attribute__((address_space(4))) uint32_t* src =
      (const __attribute__((address_space(4))) uint32_t*)(uintptr_t)src_entry;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(Entry) / 4); ++i) words[i] = src[i];
  __builtin_memcpy(&e, words, sizeof(Entry));
#else
  e = *src_entry;
#endif
}
// The slide is the last entry whose item_begin <= item (every slide has items: L_i >= 1), then (segment, head, own
// block) within it.  item derives from blockIdx alone, so the search and the entry are wave-uniform.
GP_DEV int make_view(const Args& a, int64_t item, View& w) {
  const int it = (int)item;
  int lo = 0, hi = a.nslide - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (it >= a.tab[mid].item_begin) lo = mid; else hi = mid - 1;
  }
  lo = __builtin_amdgcn_readfirstlane(lo);
  Entry e;
  load_entry_scalar(a.tab + lo, e);
  const int local = it - e.item_begin;
  const int tile = local % e.ntile;
  const int nh = local / e.ntile;
  dil_view(a, e, nh / a.H, nh % a.H, w);
  return tile;
}

GP_DEV void add_f32x4(float* p, float a, float b, float c, float d, float f) {   // read-add-write, 16-byte aligned
  f32x4* q = reinterpret_cast<f32x4*>(p);
  f32x4 x = *q;
  x[0] += a * f; x[1] += b * f; x[2] += c * f; x[3] += d * f;
  *q = x;
}

// The four k-steps of an own row as MFMA operands: lane (l32, hh) holds d = 16 ks + 8 hh .. + 7 of row l32.
struct Frag { bf16x8 f[KS]; };
GP_DEV void load_frag(Frag& r, const uint16_t* row, int hh, bool valid) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    bf16x8 z = {};
    if (valid) z = *reinterpret_cast<const bf16x8*>(row + 16 * ks + 8 * hh);
    r.f[ks] = z;
  }
}
// acc[tile row][own row] of a 32-row sub-tile: the image's rows (row-wise ds_read_b128) against an own-row fragment
GP_DEV f32x16 dot_tile(const char* img, int row, int hh, const Frag& b) {
  f32x16 acc = zero16();
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(img + row * ROWB + 32 * ks + 16 * hh);
    acc = mfma(a, b.f[ks], acc);
  }
  return acc;
}
// A operand X^T[d 32 mt + l32][tile row] of a product that contracts over 16 tile rows, by two transposed reads of
// X's row-major image: element e < 4 is tile row r16 + 4 hh + e, e >= 4 is r16 + 8 + 4 hh + e - 4 -- the rows that
// registers 8 s .. 8 s + 7 of a 32x32 C tile hold.  The 16-lane group (hh, c) reads four rows x 16 d of block
// 2 mt + c: all four blocks exist at D = 64.
GP_DEV bf16x8 read_transposed(const char* img, int r16, int mt, int lane) {
  const int hh = lane >> 5, c = (lane >> 4) & 1;
  const int blk = 2 * mt + c;
  const char* p0 = img + (r16 + 4 * hh + ((lane >> 2) & 3)) * ROWB + 32 * blk + 8 * (lane & 3);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0 + 8 * ROWB));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// LDS-DMA of two [kTile x D] images per tile.  Piece pc of the 18 goes to wave pc % NW (slot pc / NW): 64
// lane-linear 16-byte units of image pc / 9; unit u is row u / 9, chunk u % 9, and the lanes of the padding chunk
// are off.
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
// dQ (and the corrected delta): one workgroup per 256 query rows of a (slide, segment, head); K | V streamed.
__global__ __launch_bounds__(NT) void attn_bwd2_d64_dq_kernel(const Args a) {
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
  // A softmax over one key (m = 1: a one-token slide) is the constant 1, so dS is identically 0.  The packed D = 64
  // forward rounds p but not its row sum, so its o is not v in bits there and p (dP - delta) would leave a residue.
  const bool one_key = nk + vw.npad == 1;

  Dma dma;
  dma.init(w, lane, rs, rs);
  dma.load(smem, w, vw.k, rs, nk, vw.v, rs, nk);

  // Q / dO fragments (B operands: column = query l32), delta and lse of the lane's row
  Frag qf, dof, of;
  load_frag(qf, vw.q + (int64_t)i * rs, hh, i < nk);
  load_frag(dof, vw.dout + (int64_t)i * vw.rso, hh, valid);
  load_frag(of, vw.o + (int64_t)i * vw.rso, hh, valid);
  // delta: the diagonal of the four-step O.dO^T chain, summed exactly as dP sums V.dO^T.  Row n of column n is
  // register (n & 3) + 4 (n >> 3) of the lane (n, (n >> 2) & 1).
  float dl;
  {
    f32x16 dd = zero16();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) dd = mfma(of.f[ks], dof.f[ks], dd);
    const int want = (l32 & 3) + 4 * (l32 >> 3);
    float pick = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) pick = r == want ? dd[r] : pick;
    dl = __shfl(pick, l32 + 32 * ((l32 >> 2) & 1), 64);
  }
  const float lse2 = valid ? vw.lse[i] * kLog2e : INFINITY;

  // acc: dQ^T[d 32 mt + ..][q]; pk: sum_j P_ij k_j, the first-order correction of dq for the error eps of delta
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
        const f32x16 sacc = dot_tile(Kb, 32 * u + l32, hh, qf);
        const f32x16 dpacc = dot_tile(Vb, 32 * u + l32, hh, dof);
        bf16x8 dsf[2], dsl[2], pf[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float p = __builtin_amdgcn_exp2f(sacc[r] - lse2);
          if (tail) p = (kv0 + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * hh < nk) ? p : 0.f;
          const float ds = one_key ? 0.f : p * (dpacc[r] - dl);
          const uint16_t dsb = f2bf(ds);
          eps += ds;
          dsf[r >> 3][r & 7] = __builtin_bit_cast(__bf16, dsb);
          dsl[r >> 3][r & 7] = f2bf_slot(ds - bf2f(dsb));   // what the rounding of dS dropped
          pf[r >> 3][r & 7] = f2bf_slot(p);
        }
        // dQ^T[d][q] += K^T[d][key] . dS^T[key][q];  pk^T[d][q] += K^T[d][key] . P^T[key][q]
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) {
            const bf16x8 kT = read_transposed(Kb, 32 * u + 16 * s, mt, lane);
            acc[mt] = mfma(kT, dsf[s], acc[mt]);
            acc[mt] = mfma(kT, dsl[s], acc[mt]);
            pk[mt] = mfma(kT, pf[s], pk[mt]);
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
      for (int rg = 0; rg < 4; ++rg) {
        float x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = acc[mt][4 * rg + e] - pk[mt][4 * rg + e] * eps;
        add_f32x4(row + 32 * mt + 8 * rg + 4 * hh, x[0], x[1], x[2], x[3], kLn2);
      }
  }
}

// ---------------------------------------------------------------------------------------
// dK / dV: one workgroup per 256 keys of a (slide, segment, head); Q | dO + lse | delta streamed.
__global__ __launch_bounds__(NT) void attn_bwd2_d64_dkv_kernel(const Args a) {
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
  const bool one_key = nkey + vw.npad == 1;          // dS = 0 identically (see the dQ kernel)

  Dma dma;
  dma.init(w, lane, rs, rso);
  dma.load(smem, w, vw.q, rs, nkey, vw.dout, rso, nq);     // a query row past nkey is a zero pad

  // threads 0..63: lse * log2(e) (+inf past nq: P = 0), 64..127: delta (0 past nq) of tile row tid & 63, through
  // registers
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
        const f32x16 sacc = dot_tile(Qb, 32 * u + l32, hh, kf);
        const f32x16 dpacc = dot_tile(Ob, 32 * u + l32, hh, vf);
        bf16x8 pf[2], dsf[2];
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(stat + 32 * u + 8 * rg + 4 * hh);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(stat + kTile + 32 * u + 8 * rg + 4 * hh);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * rg + e;
            const float p = __builtin_amdgcn_exp2f(sacc[r] - l4[e]);   // tail query: exp2(-inf) = 0
            pf[r >> 3][r & 7] = f2bf_slot(p);
            dsf[r >> 3][r & 7] = f2bf_slot(one_key ? 0.f : p * (dpacc[r] - d4[e]));
          }
        }
        // dV^T[d][key] += dO^T[d][q] . P[q][key];  dK^T[d][key] += Q^T[d][q] . dS[q][key]
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) {
            const bf16x8 oT = read_transposed(Ob, 32 * u + 16 * s, mt, lane);
            const bf16x8 qT = read_transposed(Qb, 32 * u + 16 * s, mt, lane);
            dvacc[mt] = mfma(oT, pf[s], dvacc[mt]);
            dkacc[mt] = mfma(qT, dsf[s], dkacc[mt]);
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
      for (int rg = 0; rg < 4; ++rg) {
        const int d0 = 32 * mt + 8 * rg + 4 * hh, r = 4 * rg;
        add_f32x4(vw.gk + off + d0, dkacc[mt][r], dkacc[mt][r + 1], dkacc[mt][r + 2], dkacc[mt][r + 3], kLn2);
        add_f32x4(vw.gv + off + d0, dvacc[mt][r], dvacc[mt][r + 1], dvacc[mt][r + 2], dvacc[mt][r + 3], 1.f);
      }
  }
}

// ---------------------------------------------------------------------------------------
// Backward of the packed merge without its LayerNorm, one thread per (packed token, head): gp_attn_bwd.hip's
// merge_bwd_token arithmetic.  The slide is the last one whose first row tok0 <= token (branch 0's entries); the
// geometry and the region bases come from the (branch, slide) entries.  The branch weights (uncovered or lse == 0 ->
// -1e8, fp32 softmax over the branches) take no gradient; the sparse row whose merge slot is the token receives
// dout_b = w_b dmerged, rounded to bf16.
struct MergeArgs {
  const float* lse[GP_MAX_BRANCHES];
  uint16_t* dout[GP_MAX_BRANCHES];
  const Entry* tab;              // [nbranch][nslide]
  const uint16_t* dmerged;       // [T, H*D]
  int64_t T;
  int32_t nslide, H, nbranch;
};

__global__ __launch_bounds__(256) void merge_bwd2_d64_kernel(const MergeArgs a) {
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
  const uint16_t* dm = a.dmerged + (tok * a.H + h) * D;
  float e[GP_MAX_BRANCHES];
  uint16_t* drows[GP_MAX_BRANCHES];
  bool cov[GP_MAX_BRANCHES];
  float mx = -INFINITY;
#pragma unroll
  for (int b = 0; b < GP_MAX_BRANCHES; ++b) {
    e[b] = -1e8f; cov[b] = false; drows[b] = nullptr;
    if (b < a.nbranch) {
      const Entry& en = a.tab[(int64_t)b * a.nslide + lo];
      const GpBranch g = en.g;
      const int n = p / g.g, pt = p - n * g.g;
      const int i = pt / g.r, j = pt - i * g.r;
      cov[b] = h / g.hpg == j;
      drows[b] = a.dout[b] + en.o_off + (((int64_t)n * g.m + i) * a.H + h) * D;
      if (cov[b]) e[b] = a.lse[b][en.lse_off + ((int64_t)n * a.H + h) * g.m + i];
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
        load_e<false, 8>(dm + c, x);
        *reinterpret_cast<uint4*>(drows[b] + c) =
            make_uint4(pack2e<false>(x[0] * wb, x[1] * wb), pack2e<false>(x[2] * wb, x[3] * wb),
                       pack2e<false>(x[4] * wb, x[5] * wb), pack2e<false>(x[6] * wb, x[7] * wb));
      }
    }
}

// The one rounding of the accumulated gradients: fp32 [rows, E] planes -> bf16 dq / dk / dv rows (stride ds).
__global__ __launch_bounds__(256) void grad_store2_d64_kernel(const float* gq, const float* gk, const float* gv,
                                                              uint16_t* dq, uint16_t* dk, uint16_t* dv, int64_t ds,
                                                              int64_t rows, int E) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int cpr = E / 4;
  if (idx >= rows * cpr) return;
  const int64_t r = idx / cpr;
  const int c = (int)(idx % cpr) * 4;
  float v[4];
  load_f32<4>(gq + r * E + c, v);
  store_e<false, 4>(dq + r * ds + c, v);
  load_f32<4>(gk + r * E + c, v);
  store_e<false, 4>(dk + r * ds + c, v);
  load_f32<4>(gv + r * E + c, v);
  store_e<false, 4>(dv + r * ds + c, v);
}

// gp_varlen_bwd2_plan's buffer: this header (host side only), then the [nbranch][nslide] Entry table the kernels read
// from the device copy.  Its first fields, up to items, are public (include/gigapath_hip.h).
constexpr int32_t kMagic = 0x47504232;         // "GPB2"
struct Hdr {
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
void plan_layout(int nslide, int nbranch, Hdr& h) {
  h.tab_off = align_up((int64_t)sizeof(Hdr), 16);
  h.bytes = align_up(h.tab_off + (int64_t)nslide * nbranch * (int64_t)sizeof(Entry), 16);
}

void launch(const Hdr& h, const Entry* tab, char* ws, const uint16_t* dmerged, uint16_t* dq, uint16_t* dk, uint16_t* dv,
            int64_t ds, hipStream_t s) {
  const int E = h.H * D;
  MergeArgs m = {};
  for (int b = 0; b < h.nbranch; ++b) {
    m.lse[b] = h.lse[b];
    m.dout[b] = reinterpret_cast<uint16_t*>(ws + h.ws_dout[b]);
  }
  m.tab = tab; m.dmerged = dmerged; m.T = h.T;
  m.nslide = h.nslide; m.H = h.H; m.nbranch = h.nbranch;
  merge_bwd2_d64_kernel<<<(unsigned)((h.T * h.H + 255) / 256), 256, 0, s>>>(m);
  Args a = {};
  a.q = h.qkv; a.k = h.qkv + E; a.v = h.qkv + 2 * E;
  a.gq = reinterpret_cast<float*>(ws + h.ws_g[0]);
  a.gk = reinterpret_cast<float*>(ws + h.ws_g[1]);
  a.gv = reinterpret_cast<float*>(ws + h.ws_g[2]);
  a.row_stride = h.qkv_stride; a.nslide = h.nslide; a.H = h.H;
  for (int b = 0; b < h.nbranch; ++b) {                    // fixed order: each branch adds into the accumulators
    a.o = h.o[b];
    a.dout = m.dout[b];
    a.lse = h.lse[b];
    a.delta = reinterpret_cast<float*>(ws + h.ws_delta[b]);
    a.tab = tab + (int64_t)b * h.nslide;
    const unsigned grid = (unsigned)h.items[b];
    attn_bwd2_d64_dq_kernel<<<grid, NT, 0, s>>>(a);
    attn_bwd2_d64_dkv_kernel<<<grid, NT, 0, s>>>(a);
  }
  const int64_t n4 = h.T * (E / 4);
  grad_store2_d64_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, s>>>(a.gq, a.gk, a.gv, dq, dk, dv, ds, h.T, E);
}

}  // namespace

extern "C" int64_t gp_varlen_bwd2_plan_bytes(int nslide, int nbranch) {
  if (nslide < 1 || nbranch < 1 || nbranch > GP_MAX_BRANCHES) return -1;
  Hdr h;
  plan_layout(nslide, nbranch, h);
  return h.bytes;
}

extern "C" int gp_varlen_bwd2_plan(const int64_t* L, int nslide, int H, int Dh, const int32_t* seg_len,
                                   const int32_t* ratios, int nbranch, const uint16_t* qkv, int64_t qkv_row_stride,
                                   const uint16_t* const* o_in, const float* const* lse_in, void* plan_host,
                                   int64_t plan_bytes, int64_t* workspace_bytes) {
  GP_REQUIRE(L && seg_len && ratios && workspace_bytes, "gp_varlen_bwd2_plan: null pointer (%s)",
             !L ? "L" : !seg_len ? "seg_len" : !ratios ? "ratios" : "workspace_bytes");
  GP_REQUIRE(nslide >= 1, "gp_varlen_bwd2_plan: nslide must be >= 1 (got %d)", nslide);
  GP_REQUIRE(nbranch >= 1 && nbranch <= GP_MAX_BRANCHES, "gp_varlen_bwd2_plan: nbranch must be 1..%d (got %d)",
             GP_MAX_BRANCHES, nbranch);
  GP_REQUIRE(Dh == D, "gp_varlen_bwd2_plan: head dim D = %d unsupported (D = 64 only)", Dh);
  GP_REQUIRE(H > 0 && H <= 4096, "gp_varlen_bwd2_plan: bad H %d", H);
  const int64_t E = (int64_t)H * D;
  GP_REQUIRE(qkv_row_stride >= 3 * E && qkv_row_stride % 8 == 0,
             "gp_varlen_bwd2_plan: qkv_row_stride %lld below 3*H*D = %lld or not a multiple of 8",
             (long long)qkv_row_stride, (long long)(3 * E));
  int64_t T = 0;
  for (int i = 0; i < nslide; ++i) {
    GP_REQUIRE(L[i] > 0 && L[i] < (int64_t)0x7fffffff, "gp_varlen_bwd2_plan: slide %d has L = %lld", i, (long long)L[i]);
    T += L[i];
    GP_REQUIRE(T < (int64_t)0x7fffffff, "gp_varlen_bwd2_plan: %lld packed tokens exceed 2^31 - 1", (long long)T);
  }
  GP_REQUIRE((T * H + 255) / 256 < (int64_t)0x7fffffff && (T * (E / 4) + 255) / 256 < (int64_t)0x7fffffff,
             "gp_varlen_bwd2_plan: T*H*D too large for one launch");
  Hdr h;
  memset(&h, 0, sizeof(h));
  plan_layout(nslide, nbranch, h);
  uint64_t off = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t at = off;
    off += (bytes + 255) / 256 * 256;
    return (int64_t)at;
  };
  for (int b = 0; b < nbranch; ++b) {
    GP_REQUIRE(seg_len[b] > 0 && ratios[b] > 0, "gp_varlen_bwd2_plan: branch %d: bad seg_len %d / ratio %d", b, seg_len[b],
               ratios[b]);
    // a tile's 64 gathered rows are addressed by 32-bit byte offsets from the tile's first row
    GP_REQUIRE(qkv_row_stride * ratios[b] * 2 * kTile < (int64_t)0x7fffffff,
               "gp_varlen_bwd2_plan: branch %d: qkv_row_stride %lld x ratio %d too large for a tile's 32-bit offsets", b,
               (long long)qkv_row_stride, ratios[b]);
    uint64_t rows = 0;                                      // (sparse row, head)s of every slide
    int64_t items = 0;
    for (int i = 0; i < nslide; ++i) {
      const GpBranch g = gp_make_branch(L[i], seg_len[b], ratios[b], H);
      rows += (uint64_t)g.nseg * g.m * H;
      items += (int64_t)g.nseg * H * ((g.m + kOwn - 1) / kOwn);
      GP_REQUIRE(items < (int64_t)0x7fffffff, "gp_varlen_bwd2_plan: branch %d: %lld work items exceed one launch", b,
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

  GP_REQUIRE(plan_bytes >= h.bytes, "gp_varlen_bwd2_plan: plan buffer %lld < %lld bytes (gp_varlen_bwd2_plan_bytes)",
             (long long)plan_bytes, (long long)h.bytes);
  GP_REQUIRE(gp_aligned(plan_host, 8), "gp_varlen_bwd2_plan: misaligned pointer (plan_host, 8 bytes)");
  GP_REQUIRE(qkv != nullptr && o_in != nullptr && lse_in != nullptr, "gp_varlen_bwd2_plan: null pointer (%s)",
             !qkv ? "qkv" : !o_in ? "o_in" : "lse_in");
  GP_REQUIRE(gp_aligned(qkv, 16), "gp_varlen_bwd2_plan: misaligned pointer (qkv)");
  for (int b = 0; b < nbranch; ++b) {
    GP_REQUIRE(o_in[b] != nullptr && lse_in[b] != nullptr, "gp_varlen_bwd2_plan: null pointer (o_in / lse_in [%d])", b);
    GP_REQUIRE(gp_aligned(o_in[b], 16) && gp_aligned(lse_in[b], 4),
               "gp_varlen_bwd2_plan: misaligned pointer (o_in / lse_in [%d])", b);
  }
  char* base = static_cast<char*>(plan_host);
  memset(base, 0, (size_t)h.bytes);
  Entry* tab = reinterpret_cast<Entry*>(base + h.tab_off);
  for (int b = 0; b < nbranch; ++b) {
    int64_t tok = 0, oo = 0, lo = 0, items = 0;
    for (int i = 0; i < nslide; ++i) {
      Entry& e = tab[(size_t)b * nslide + i];
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
  h.magic = kMagic;
  h.nslide = nslide; h.nbranch = nbranch; h.H = H; h.D = D;
  h.T = T;
  h.qkv_stride = qkv_row_stride;
  h.qkv = qkv;
  memcpy(base, &h, sizeof(h));
  return 0;
}

extern "C" int gp_dilated_attn_bwd2_varlen(const void* plan_host, const void* plan_dev, const uint16_t* dmerged,
                                           uint16_t* dq, uint16_t* dk, uint16_t* dv, int64_t d_row_stride,
                                           void* workspace, size_t workspace_bytes, int q_log2_prescaled, int fmt,
                                           void* stream) {
  GP_REQUIRE(fmt == GP_FMT_BF16, "gp_dilated_attn_bwd2_varlen: bad fmt %d (GP_FMT_BF16 only)", fmt);
  GP_REQUIRE(q_log2_prescaled,
             "gp_dilated_attn_bwd2_varlen: q_log2_prescaled must be 1 (q pre-scaled by D^-0.5 log2 e)");
  GP_REQUIRE(plan_host != nullptr && plan_dev != nullptr, "gp_dilated_attn_bwd2_varlen: null pointer (%s)",
             !plan_host ? "plan_host" : "plan_dev");
  GP_REQUIRE(gp_aligned(plan_host, 8) && gp_aligned(plan_dev, 16),
             "gp_dilated_attn_bwd2_varlen: misaligned pointer (plan_host 8 bytes / plan_dev 16 bytes)");
  Hdr h;
  memcpy(&h, plan_host, sizeof(h));
  GP_REQUIRE(h.magic == kMagic, "gp_dilated_attn_bwd2_varlen: not a gp_varlen_bwd2_plan buffer");
  GP_REQUIRE(h.D == D && h.nslide >= 1 && h.nbranch >= 1 && h.nbranch <= GP_MAX_BRANCHES && h.H > 0 && h.T > 0 &&
                 h.T < (int64_t)0x7fffffff,
             "gp_dilated_attn_bwd2_varlen: corrupt plan header");
  const void* ptrs[] = {dmerged, dq, dk, dv};
  const char* names[] = {"dmerged", "dq", "dk", "dv"};
  for (int i = 0; i < 4; ++i) {
    GP_REQUIRE(ptrs[i] != nullptr, "gp_dilated_attn_bwd2_varlen: null pointer (%s)", names[i]);
    GP_REQUIRE(gp_aligned(ptrs[i], 16), "gp_dilated_attn_bwd2_varlen: misaligned pointer (%s)", names[i]);
  }
  const int64_t E = (int64_t)h.H * h.D;
  GP_REQUIRE(d_row_stride >= E && d_row_stride % 8 == 0,
             "gp_dilated_attn_bwd2_varlen: d_row_stride %lld below H*D = %lld or not a multiple of 8",
             (long long)d_row_stride, (long long)E);
  GP_REQUIRE(workspace != nullptr && workspace_bytes >= (size_t)h.ws_total,
             "gp_dilated_attn_bwd2_varlen: workspace too small (%zu bytes, gp_varlen_bwd2_plan asks %zu)",
             workspace ? workspace_bytes : (size_t)0, (size_t)h.ws_total);
  GP_REQUIRE(gp_aligned(workspace, 16), "gp_dilated_attn_bwd2_varlen: misaligned workspace (16 bytes)");
  for (int b = 0; b < h.nbranch; ++b)
    GP_REQUIRE(h.items[b] > 0 && h.items[b] < (int64_t)0x7fffffff,
               "gp_dilated_attn_bwd2_varlen: branch %d: %lld work items exceed one launch", b, (long long)h.items[b]);

  char* ws = static_cast<char*>(workspace);
  const Entry* tab = reinterpret_cast<const Entry*>(static_cast<const char*>(plan_dev) + h.tab_off);
  hipStream_t s = gp_stream(stream);
  // the accumulators start at zero: a (token, head) no branch covers keeps it
  const hipError_t me = hipMemsetAsync(ws + h.ws_g[0], 0, (size_t)(h.ws_total - h.ws_g[0]), s);
  if (me != hipSuccess) {
    gp_set_error("gp_dilated_attn_bwd2_varlen: hipMemsetAsync: %s", hipGetErrorString(me));
    return (int)me;
  }
  launch(h, tab, ws, dmerged, dq, dk, dv, d_row_stride, s);
  return gp_check_launch("gp_dilated_attn_bwd2_varlen");
}
