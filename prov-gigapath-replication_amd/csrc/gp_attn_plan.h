// What the attention unit (gp_attn.hip) and the merge unit (gp_merge.hip) share: the scalar-unit division,
// the per-branch entries of their launch arguments and work tables, and the varlen plan's layout (written by
// gp_varlen_plan, read by both units' varlen launches).
#pragma once
#include "gp_api.h"
#include "gp_common.h"

// Exact unsigned division by a launch constant d < 2^31 via a multiply-high: the merge kernel's
// per-token divisions are wave-uniform, so they run on the scalar unit instead of ~25 VALU
// instructions each.  With m = floor(2^32 (2^l - d) / d) + 1, l = ceil(log2 d), the quotient is
// (mulhi(n, m) + n) >> l for every n < 2^31 (mulhi(n, m) < n, so the sum cannot wrap); d == 1 is
// m = 0, l = 0 -- no branch, so a chain of divisions does not split the scalar argument loads
// into one wait per division.
struct DivMagic {
  uint32_t m;
  int32_t l;     // 0: d == 1
};
inline DivMagic make_div_magic(uint32_t d) {
  DivMagic r{0, 0};
  if (d <= 1) return r;
  int l = 0;
  while ((1ull << l) < d) ++l;                                   // ceil(log2 d)
  r.m = (uint32_t)(((((uint64_t)1 << l) - d) << 32) / d + 1);
  r.l = l;
  return r;
}
GP_DEV uint32_t div_magic(uint32_t n, DivMagic mg) {   // n < 2^31
  return (__umulhi(n, mg.m) + n) >> mg.l;
}

struct AttnBranch {
  GpBranch g;
  int32_t nqb;          // q-blocks per (batch-segment, head)
  int32_t n_lo;         // first segment whose dense slots meet the query window
  int32_t nseg_w;       // segments meeting the window
  int32_t kv_sparse;    // 0: head h at columns h*D of a k/v row; 1: at (h % hpg)*D (sparsified rows)
  int64_t item_begin;   // first work item of this branch
  const uint16_t* k;    // key rows: token t of batch b at row (b*L + t - kv_tok_base)
  const uint16_t* v;
  int64_t kv_stride;    // elements between consecutive k / v rows
  int64_t kv_tok_base;
  uint16_t* o;          // [B*nseg, m, H, D]
  float* lse;           // [B*nseg, H, m]
  int32_t kpart, kparts;   // key part kpart of kparts (<= 1: all keys; see GpAttnBranch.key_parts)
  // varlen table entries only (one per (slide, branch); B = 1, window = the whole slide)
  const uint16_t* q;    // the slide's first query row
  int64_t L;            // the slide's length (CLS + tiles)
  DivMagic d_nqb, d_nsegw, d_hpg, d_r;   // the work-item decode's divisors (scalar multiply-high)
};
inline void attn_branch_magic(AttnBranch& e) {
  e.d_nqb = make_div_magic((uint32_t)e.nqb);
  e.d_nsegw = make_div_magic((uint32_t)e.nseg_w);
  e.d_hpg = make_div_magic((uint32_t)e.g.hpg);
  e.d_r = make_div_magic((uint32_t)e.g.r);
}

struct MergeBranch {
  GpBranch g;
  const uint16_t* o;
  const float* lse;
  DivMagic dg, dr;   // division by g.g and by g.r
};
inline void merge_branch_magic(MergeBranch& m) {
  m.dg = make_div_magic((uint32_t)m.g.g);
  m.dr = make_div_magic((uint32_t)m.g.r);
}

// Varlen packing (config C5): several slides concatenated token-major in one [T, 3E] qkv buffer
// (slide i at rows [tok_off[i], tok_off[i] + L_i)), one attention launch and one merge launch
// for all of them.  Every slide keeps its own segment schedule (s = min(sl, L_i), ...) and no
// query attends across slides, so each slide's outputs are those of its own B = 1 forward.
// The plan (host bytes, copied by the caller to device memory) holds the work table.
constexpr int32_t kVarlenMagic = 0x47505631;   // "GPV1"
struct VarlenHdr {
  int32_t magic, nslide, nbranch, H, D, ntab;
  int64_t T, total_items, qkv_stride;
  int64_t tab_off, mtab_off, tok_off_off, bytes;
};
inline int64_t gp_align16(int64_t x) { return (x + 15) & ~int64_t(15); }
inline void varlen_layout(int nslide, int nbranch, VarlenHdr& h) {
  h.tab_off = gp_align16(sizeof(VarlenHdr));
  h.mtab_off = gp_align16(h.tab_off + (int64_t)nslide * nbranch * sizeof(AttnBranch));
  h.tok_off_off = gp_align16(h.mtab_off + (int64_t)nslide * nbranch * sizeof(MergeBranch));
  h.bytes = gp_align16(h.tok_off_off + (int64_t)(nslide + 1) * sizeof(int64_t));
}

// per-device cache of the CU count (defined in gp_attn.hip)
int attn_num_cus(hipStream_t s);
