// What the two forward attention kernels (attention.hip: one workgroup per head, T <= 272; attention_long.hip: tiled,
// T <= 1024) share: the position scheme of the logits.  Both kernels hold S^T = K Q^T in 16x16x32 MFMA accumulators:
// lane (li = lane & 15, g = lane >> 4) owns query column li and, of every 16-key tile, the keys 4 g + {0..3}.  A new
// position scheme, or a new patch grid rule, is written here once.  The Q-fragment load and the output-tile store are
// NOT here: each is the same text in both kernels, but through a shared helper it moved a schedule (see attention.hip).
//
// AttnPos::RelBias: BEiT's learned relative-position bias.  The logit of query i and key j is
//   fp32(q_i . k_j) * scale + table[idx(i, j)][h],  table [R, H] fp32, R = (2 gh - 1)(2 gw - 1) + 3,
// token 0 = CLS, patch p at (y, x) = ((p - 1) / gw, (p - 1) % gw).  No [T, T] bias exists anywhere: the head's column
// of the table is staged in LDS next to koff[key] = y_k (2 gw - 1) + x_k of every patch key, and a lane forms
//   idx = (y_q + gh - 1)(2 gw - 1) + x_q + gw - 1 - koff[key]
// per logit (one division per lane and query tile).  A CLS query reads row R - 3 (R - 1 against the CLS key), a patch
// query row R - 2 against the CLS key.
//
// AttnPos::Rope: the rotary embedding of EVA-02 / DINOv3.  q and k of token t are rotated pairwise,
//   (x[2i], x[2i+1]) -> (x[2i] c - x[2i+1] s, x[2i+1] c + x[2i] s),  (c, s) = table[t][i],  table [T, hd / 2, 2] fp32,
// before the logits are formed; v is untouched.  A 16-byte chunk holds four whole pairs, so a chunk is rotated in
// registers between its global load and its use (rope_chunk, basd_frag.h: fp32 arithmetic, one rounding to bf16); its
// eight table floats are two 16-byte loads issued next to it.  The kernels know no grid: row t belongs to token t (the
// host writes (1, 0) into the rows of tokens that are not rotated).
//
// Legal combinations (attn_pos_ok): a position scheme needs head dim 64 (whole 32-deep steps, the table sizes below)
// and comes with the CLS tap only -- no query-mean tap, no LSE output.
#pragma once
#include "basd_frag.h"

namespace basd {

enum class AttnPos { None, RelBias, Rope };

struct AttnPosArg {
  const float* table;                                // RelBias: [R, H] fp32, heads on the fast axis; Rope: [T, hd / 2, 2]
  int gh, gw;                                        // RelBias: patch grid, T = gh * gw + 1; otherwise 0
};

template <AttnPos POS, int HD, bool QMEAN = false>
constexpr bool attn_pos_ok = POS == AttnPos::None || (HD == 64 && !QMEAN);

// ---------------------------------------------------------------------------------------------- relative bias ----
__device__ __forceinline__ int relbias_rows(const AttnPosArg& pos) { return (2 * pos.gh - 1) * (2 * pos.gw - 1) + 3; }

// koff[key]: y_k (2 gw - 1) + x_k of a patch key, 0 for the CLS and the padding keys (overridden / masked).  The copy of
// the head's column into LDS next to it is each kernel's own: the short kernel stores the raw column in one batch of
// loads, the long one the column divided by scale in batches of four (one staging helper for both put the short
// 17-tile instantiation above the timing band: profiles/attention_pos_one_copy_ab.txt).
__device__ __forceinline__ int relbias_koff(const AttnPosArg& pos, int key, int T) {
  const int yk = (key >= 1 && key < T) ? (key - 1) / pos.gw : 0;
  return (key >= 1 && key < T) ? yk * (2 * pos.gw - 1) + (key - 1 - yk * pos.gw) : 0;
}

// The constants of a lane's query qi: a patch query reads tab[qb - koff[key]], a CLS query the constant row qb = R - 3
// (a padding query too: any valid index will do); against the CLS key both read row c0.
struct RelBiasQuery {
  int qb, c0;
  bool patch;
};
__device__ __forceinline__ RelBiasQuery relbias_query(const AttnPosArg& pos, int qi, int T) {
  const int R = relbias_rows(pos), rl = 2 * pos.gw - 1;
  RelBiasQuery q;
  q.patch = qi >= 1 && qi < T;
  const int yq = q.patch ? (qi - 1) / pos.gw : 0;
  q.qb = q.patch ? (yq + pos.gh - 1) * rl + (qi - 1 - yq * pos.gw) + pos.gw - 1 : R - 3;
  q.c0 = q.patch ? R - 2 : R - 1;
  return q;
}

// The lane's four table entries of one 16-key tile: koff_tile = koff + the tile's first key, keys 4 g + {0..3};
// first_tile: the tile starts at key 0, whose first key is the CLS token.  (attention.hip writes this loop out on the
// same RelBiasQuery: see there.)
__device__ __forceinline__ void relbias_gather(const RelBiasQuery& q, const float* tab, const int* koff_tile, int g,
                                               bool first_tile, float (&bias)[4]) {
  const int4 ko = *reinterpret_cast<const int4*>(koff_tile + 4 * g);
  const int kk[4] = {ko.x, ko.y, ko.z, ko.w};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int idx = q.patch ? q.qb - kk[r] : q.qb;
    if (first_tile && r == 0 && g == 0) idx = q.c0;
    bias[r] = tab[idx];
  }
}

// ----------------------------------------------------------------------------------------------------- rotary ----
// (cos, sin) of the four pairs of the chunk at channel col of a token: call inside the bounds guard of the chunk's own
// load; rope_none for a chunk outside it (zeros stay zeros under the rotation)
__device__ __forceinline__ void rope_rows(const float* table, int token, int hd, int col, float4 (&cs)[2]) {
  const float4* p = reinterpret_cast<const float4*>(table + (size_t)token * hd + col);
  cs[0] = p[0];
  cs[1] = p[1];
}
__device__ __forceinline__ void rope_none(float4 (&cs)[2]) { cs[0] = cs[1] = make_float4(0.f, 0.f, 0.f, 0.f); }

}  // namespace basd
