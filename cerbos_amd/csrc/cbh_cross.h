// Cross-product batches built on the device (cerbos_hip.h cbh_batch_upload_cross) and the allow bitmap of a resident batch
// (cbh_result_download_allow_bits).  Three small kernels, none of them on the decision path: the product they build is an ordinary
// resident batch the decision kernels read unchanged.  And the two kernels of the DIRECT road (cbh_cross_upload_ex) - the one lane that
// writes the action words, and the gather that turns chosen pairs of a set into a resident batch (cbh_cross_pairs_upload) -, which
// materialises no product: its decision kernels are the flat kernels' CROSS instantiations (cbh_check_flat.h), which read the
// halves' compact form in place and write ballots.  And the lane per principal that writes a wide set's role words.  And, at the
// end, the kernels of cbh_cross_review, which reduce a tile's ballot planes to counts and an ordered list of pairs on the device.
//
// The product's layout: N principals x M resources, resource-major.  Device request q = j' * N + i' pairs the
// j'-th resource with the i'-th principal of the caller's orders; the halves batch holds the N principals in its first N
// requests and the M resources in its last M.  Roles, heap and strings are the halves' own arrays, shared by every request.
#pragma once
#include "cbh_interp.h"

struct CrossArgs {
  // the halves as uploaded: [CBH_RQ_NFIELDS][nh], [n_columns][nh], [n_columns][nh], nh = n + m
  const CBH_G u32* h_req; const CBH_G u8* h_tag; const CBH_G u64* h_val;
  const CBH_G u32* p_order; const CBH_G u32* r_order;   // [n], [m], or null = identity
  const CBH_G u8* col_side;                             // [n_columns] 1 = the column travels with the resource (root R.attr), 0 = with the principal
  const CBH_G u32* action_ids;                          // [a]
  CBH_G u32* req; CBH_G u8* tag; CBH_G u64* val;        // the product: [CBH_RQ_NFIELDS][nm], [n_columns][nm], [n_columns][nm]
  CBH_G u32* tuple_action;                              // [nm * a]
  u32 n, m, a, n_columns;
};

// which half a request field comes from: bit f set = the resource's (cerbos_amd/cross.py R_FIELDS); ACT_OFF / ACT_CNT are computed
#define CBH_CROSS_R_FIELDS ((1u << CBH_RQ_KIND) | (1u << CBH_RQ_R_SCOPE) | (1u << CBH_RQ_R_VERSION) | (1u << CBH_RQ_S_RESOURCE_ID) | \
                            (1u << CBH_RQ_S_KIND) | (1u << CBH_RQ_S_R_SCOPE) | (1u << CBH_RQ_S_R_VERSION))

// One lane per device request.  Consecutive lanes are consecutive principals of one resource: principal-side loads are coalesced
// (or a gather through p_order out of N rows that stay in cache), resource-side loads hit one or two rows per wave, and every
// store goes to [field or column][q] - 64 consecutive elements per wave instruction.  A pure stream: nm * (64 + 9 * n_columns) bytes out.
__global__ __launch_bounds__(256) void cbh_cross_expand_kernel(CrossArgs x) {
  const u64 q64 = (u64)blockIdx.x * 256u + threadIdx.x;   // (n * m may lie within a workgroup of 2^32)
  const u32 nm = x.n * x.m;
  if (q64 >= nm) return;
  const u32 q = (u32)q64;
  const u32 jp = q / x.n, ip = q - jp * x.n;
  const size_t NH = (size_t)x.n + x.m, NM = nm;
  const size_t pi = x.p_order ? x.p_order[ip] : ip;                    // the principal's row of the halves
  const size_t ri = (size_t)x.n + (x.r_order ? x.r_order[jp] : jp);    // the resource's
#pragma unroll
  for (u32 f = 0; f < CBH_RQ_NFIELDS; ++f) {
    u32 v;
    if (f == CBH_RQ_ACT_OFF) v = q * x.a;
    else if (f == CBH_RQ_ACT_CNT) v = x.a;
    else v = x.h_req[f * NH + (((CBH_CROSS_R_FIELDS >> f) & 1u) ? ri : pi)];
    x.req[f * NM + q] = v;
  }
  for (u32 c = 0; c < x.n_columns; ++c) {
    const size_t src = c * NH + (x.col_side[c] ? ri : pi);
    x.tag[c * NM + q] = x.h_tag[src];
    x.val[c * NM + q] = x.h_val[src];
  }
}

// tuple_action = the A ids repeated nm times: one lane per four words, a 16-byte store each (the array starts a device allocation,
// so word 4 t is 16-byte aligned); the last lane writes what is left word by word.
__global__ __launch_bounds__(256) void cbh_cross_actions_kernel(CrossArgs x) {
  const u64 total = (u64)x.n * x.m * x.a;
  const u64 w = ((u64)blockIdx.x * 256u + threadIdx.x) * 4u;
  if (w >= total) return;
  u32 k = (u32)(w % x.a);
  u32 v[4];
  for (u32 e = 0; e < 4; ++e) { v[e] = x.action_ids[k]; k = k + 1u == x.a ? 0u : k + 1u; }
  if (w + 4u <= total) {
    uint4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
    *reinterpret_cast<CBH_G uint4*>(x.tuple_action + w) = o;
  } else {
    for (u32 e = 0; w + e < total; ++e) x.tuple_action[w + e] = v[e];
  }
}

// The allow bitmap: bit k of bits[k >> 6] = tuple k's effect is CBH_EFFECT_ALLOW.  One lane per tuple; the effect comes from the
// packed result word where the last launch wrote that form (`packed`, cbh_pk_effect), else from the effect bytes; the wave ballots
// and its first lane stores the word.  Lanes behind the last tuple vote no, so the last word's unused bits are 0.  Every lane
// reaches the ballot (cbh_interp.h's discipline).
struct AllowBitsArgs { const CBH_G u32* packed; const CBH_G u8* effect; CBH_G u64* bits; u32 n_tuples; u32 pad; };
__global__ __launch_bounds__(256) void cbh_allow_bits_kernel(AllowBitsArgs a) {
  const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
  u32 eff = 0;
  if (k < a.n_tuples) eff = a.packed ? cbh_pk_effect(a.packed[k]) : (u32)a.effect[k];
  const u64 mask = wave_ballot(eff == CBH_EFFECT_ALLOW);
  if ((threadIdx.x & 63u) == 0u && k < a.n_tuples) a.bits[k >> 6] = mask;
}

// The direct road's action words (CrossDev.act_word), one per group of four actions (a set of A actions is decided in (A + 3) / 4
// launches, group g = the actions 4 g .. 4 g + 3): the classes of the group's actions, by the expressions of cbh_compact_pack_kernel
// (clamps included), five bits each as in word 3 of a compact record, and the group's action count << 20.  One lane, once per upload.
struct CrossActWordArgs { const CBH_G u32* action_ids; const CBH_G u8* action_class; CBH_G u32* out; u32 a, K; };
__global__ __launch_bounds__(64) void cbh_cross_act_word_kernel(CrossActWordArgs x) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const u32 kmax = x.K ? x.K - 1u : 0u;
  for (u32 g = 0; 4u * g < x.a; ++g) {
    const u32 cnt = x.a - 4u * g < 4u ? x.a - 4u * g : 4u;
    u32 w = cnt << 20;
    for (u32 k = 0; k < 4; ++k) {
      const u32 aid = x.action_ids[4u * g + (k < cnt ? k : 0u)];
      const u32 ca = x.K ? x.action_class[aid < x.K ? aid : kmax] : 31u;
      w |= ((k < cnt && aid < x.K && ca < 31u) ? ca : 31u) << (5u * k);
    }
    x.out[g] = w;
  }
}

// The direct road's role words (CrossRoleGroup.role_words / rc_all) of a set whose principals have up to CBH_CX_MAX_ROLES roles (cerbos_hip.h
// CBH_CX_ROLE_GROUPS): the compact record of a principal holds its first four roles - group 0 - and per further group g the word
// words[(g - 1) * n + row] holds the classes of its roles 4 g .. 4 g + 3 and their count, in the action words' format; all[row] is
// the OR of 1 << class over ALL of its roles.  The classes by cbh_compact_pack_kernel's rule.  `role_off` is the halves' own request
// word, `role_cnt` the principals' TRUE counts (the uploaded request words hold them clamped to four).  One lane per principal's
// row, once per upload; the host has checked every slice against n_roles.
struct CrossRoleWordArgs {
  const CBH_G u32* role_off; const CBH_G u32* role_cnt; const CBH_G u32* roles; const CBH_G u8* role_class;
  CBH_G u32* words; CBH_G u32* all;
  u32 n, groups, K, pad;
};
__global__ __launch_bounds__(256) void cbh_cross_role_word_kernel(CrossRoleWordArgs x) {
  const u64 r64 = (u64)blockIdx.x * 256u + threadIdx.x;
  if (r64 >= x.n) return;
  const u32 r = (u32)r64;
  const u32 kmax = x.K ? x.K - 1u : 0u;
  const u32 off = x.role_off[r], total = x.role_cnt[r];
  u32 all = 0, w = 0;
  for (u32 i = 0; i < 4u * x.groups; ++i) {
    const u32 g = i >> 2, k = i & 3u;
    if (k == 0) w = (total > 4u * g ? (total - 4u * g < 4u ? total - 4u * g : 4u) : 0u) << 20;
    u32 cls = 31u;
    if (i < total) {
      const u32 rid = x.roles[off + i];
      const u32 cr = x.K ? x.role_class[rid < x.K ? rid : kmax] : 31u;
      cls = (rid < x.K && cr < 31u) ? cr : 31u;
      all |= 1u << cls;
    }
    w |= cls << (5u * k);
    if (k == 3u && g >= 1u) x.words[(size_t)(g - 1u) * x.n + r] = w;
  }
  x.all[r] = all;
}

// Chosen pairs of a direct set as an ordinary resident batch (cerbos_hip.h cbh_cross_pairs_upload): cbh_cross_expand_kernel for a LIST of
// pairs.  Request q pairs device principal pair_p[q] with device resource pair_r[q] - the set's own orders, what a tile's bit index
// decodes to - instead of dividing q; the host has checked every index against n and m before the launch.  One lane per pair; the
// loads gather from the N + M rows (which stay in cache), every store goes to [field or column][q].  cbh_cross_actions_kernel then
// fills tuple_action as for a product of n_pairs x 1.
struct CrossGatherArgs {
  const CBH_G u32* h_req; const CBH_G u8* h_tag; const CBH_G u64* h_val;   // the set's halves: [CBH_RQ_NFIELDS][nh], [n_columns][nh], [n_columns][nh]
  const CBH_G u32* p_order; const CBH_G u32* r_order;                      // [n], [nh - n], or null = identity
  const CBH_G u8* col_side;                                                // [n_columns]
  const CBH_G u32* pair_p; const CBH_G u32* pair_r;                        // [n_pairs] device indices, < n and < nh - n
  CBH_G u32* req; CBH_G u8* tag; CBH_G u64* val;                           // the batch: [CBH_RQ_NFIELDS][n_pairs], [n_columns][n_pairs] twice
  u32 n, nh, n_pairs, a, n_columns, pad;
  const CBH_G u32* p_role_cnt;                                             // [n] the principals' true role counts by halves row, or null = the request words' (a set with role groups uploads those clamped)
};
__global__ __launch_bounds__(256) void cbh_cross_gather_kernel(CrossGatherArgs x) {
  const u64 q64 = (u64)blockIdx.x * 256u + threadIdx.x;
  if (q64 >= x.n_pairs) return;
  const u32 q = (u32)q64;
  const u32 ip = x.pair_p[q], jp = x.pair_r[q];
  const size_t NH = x.nh, NP = x.n_pairs;
  const size_t pi = x.p_order ? x.p_order[ip] : ip;
  const size_t ri = (size_t)x.n + (x.r_order ? x.r_order[jp] : jp);
#pragma unroll
  for (u32 f = 0; f < CBH_RQ_NFIELDS; ++f) {
    u32 v;
    if (f == CBH_RQ_ACT_OFF) v = q * x.a;
    else if (f == CBH_RQ_ACT_CNT) v = x.a;
    else if (f == CBH_RQ_ROLE_CNT && x.p_role_cnt) v = x.p_role_cnt[pi];
    else v = x.h_req[f * NH + (((CBH_CROSS_R_FIELDS >> f) & 1u) ? ri : pi)];
    x.req[f * NP + q] = v;
  }
  for (u32 c = 0; c < x.n_columns; ++c) {
    const size_t src = c * NH + (x.col_side[c] ? ri : pi);
    x.tag[c * NP + q] = x.h_tag[src];
    x.val[c * NP + q] = x.h_val[src];
  }
}

// ---- The review of a direct set (cerbos_hip.h cbh_cross_review): a tile's planes reduced where the `_x` kernels left them -------
// The planes of a tile of mt resources are [kinds][a][words] ballot words (kinds = 1: allow only, 2: allow | flagged), bit
// q = j * n + i' of a plane = resource j of the tile, principal i'.  Nothing here decides anything: these kernels read the planes
// once each and write counters and a list, so that no plane has to cross the host link.  All sums are integer sums: exact, and
// independent of the order the workgroups arrive in.  Where the simulator's runtime lacks an operation (it has atomicOr only),
// the difference stays under CBH_HOSTSIM in cx_add32 below.
__device__ __forceinline__ void cx_add32(CBH_G u32* p, u32 v) {
#ifndef CBH_HOSTSIM
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *p += v;   // (the simulator runs one lane at a time)
#endif
}
// exclusive prefix and total of a per-lane count below 2^bits over the wave, by bit planes; every lane of the wave reaches it
__device__ __forceinline__ u64 cx_wave_prefix(u64 x, u32 bits, u32 lane, u64& total) {
  u64 pre = 0; total = 0;
  const u64 lt = (1ull << lane) - 1ull;
  for (u32 b = 0; b < bits; ++b) {
    const u64 mk = wave_ballot(((x >> b) & 1ull) != 0ull);
    pre += (u64)__builtin_popcountll(mk & lt) << b;
    total += (u64)__builtin_popcountll(mk) << b;
  }
  return pre;
}

struct CrossReviewArgs {
  const CBH_G u64* planes;   // [kinds][a][words]: the tile's
  CBH_G u32* by_r;           // [kinds][a][mr] counts per resource of the call's range; this tile writes the columns [j0, j0 + mt)
  CBH_G u32* by_p;           // [kinds][a][n] counts per principal, accumulated over the call's tiles (zeroed before the first)
  u32 n, mt, a, kinds;
  u32 words, mr, j0, grid;   // `grid`: the launch's workgroups (the kernels stride by it)
  u32 g, bits;               // rows kernel: lanes per resource (a power of two, at most 64) and the bits of a lane's largest count
  u32 strip, pad;            // columns kernel: resources per strip
};

// Per-resource counts: a segmented popcount over the bit ranges [j * n, (j + 1) * n) of every plane.  A range starts and ends
// anywhere in a word: its first and last word are masked (one word may be both, and holds many resources where n < 64; the plane's
// last word is partial, its unused bits are 0 and lie outside every range anyway).  `g` lanes share a resource and stride over its
// words - consecutive lanes read consecutive words -; their counts are summed by ballots over the group's lanes, and the group's
// first lane stores the sum: every count of a tile is written exactly once, so by_r needs no zeroing.  Every lane of a workgroup
// makes the same number of rounds and reaches every ballot; lanes behind the last segment count nothing.
__global__ __launch_bounds__(256) void cbh_cross_review_rows_kernel(CrossReviewArgs x) {
  const u32 lane = threadIdx.x & 63u;
  const u32 g = x.g, sub = lane & (g - 1u);
  const u64 gmask = (g >= 64u ? ~0ull : (1ull << g) - 1ull) << (lane - sub);
  const u32 per_block = 256u / g;
  const u64 nseg = (u64)x.kinds * x.a * x.mt;
  for (u64 blk = blockIdx.x; blk * per_block < nseg; blk += x.grid) {
    const u64 seg = blk * per_block + threadIdx.x / g;
    const bool live = seg < nseg;
    u32 plane = 0, j = 0, cnt = 0;
    if (live) {
      plane = (u32)(seg / x.mt); j = (u32)(seg - (u64)plane * x.mt);
      const u64 lo = (u64)j * x.n, hi = lo + x.n;   // (n * mt < 2^32)
      const u64 w_lo = lo >> 6, w_hi = (hi - 1u) >> 6;
      const CBH_G u64* w = x.planes + (size_t)plane * x.words;
      for (u64 i = w_lo + sub; i <= w_hi; i += g) {
        u64 v = w[i];
        if (i == w_lo) v &= ~0ull << (lo & 63u);
        if (i == w_hi && (hi & 63u)) v &= ~0ull >> (64u - (u32)(hi & 63u));
        cnt += (u32)__builtin_popcountll(v);
      }
    }
    u32 total = cnt;
    if (g > 1u) {
      total = 0;
      for (u32 b = 0; b < x.bits; ++b) {
        const u64 mk = wave_ballot(((cnt >> b) & 1u) != 0u);
        total += (u32)__builtin_popcountll(mk & gmask) << b;
      }
    }
    if (live && sub == 0u) x.by_r[(size_t)plane * x.mr + x.j0 + j] = total;
  }
}

// Per-principal counts: the column sums of a plane read as an mt x n bit matrix whose rows are n bits apart.  A wave takes 64
// columns of a strip of `strip` resources, a lane per column: it walks the strip's rows - the wave's lanes read the one or two
// words that hold their 64 bits of the row -, sums its column in a register, and adds the sum to by_p with ONE atomic per
// destination: a wave instruction adds to 64 consecutive counters.  The units are ordered columns-first, so the four waves of a
// workgroup hold different columns of one strip wherever n > 192: one atomic per destination and workgroup.  A column without a
// set bit in the strip adds nothing (the flagged planes are mostly empty).  No ballot, no barrier.
__global__ __launch_bounds__(256) void cbh_cross_review_cols_kernel(CrossReviewArgs x) {
  const u32 lane = threadIdx.x & 63u;
  const u32 chunks = (x.n + 63u) / 64u, strips = (x.mt + x.strip - 1u) / x.strip;
  const u64 units = (u64)x.kinds * x.a * strips * chunks;
  for (u64 u = (u64)blockIdx.x * 4u + threadIdx.x / 64u; u < units; u += (u64)x.grid * 4u) {
    const u32 c = (u32)(u % chunks);
    const u64 r = u / chunks;
    const u32 s = (u32)(r % strips), plane = (u32)(r / strips);
    const u32 i = c * 64u + lane;
    if (i >= x.n) continue;
    const CBH_G u64* w = x.planes + (size_t)plane * x.words;
    u32 j = s * x.strip;
    const u32 j_end = j + x.strip < x.mt ? j + x.strip : x.mt;
    u64 bit = (u64)j * x.n + i;
    u32 cnt = 0;
#pragma unroll 8
    for (; j < j_end; ++j, bit += x.n) cnt += (u32)(w[bit >> 6] >> (bit & 63u)) & 1u;
    if (cnt) cx_add32(x.by_p + (size_t)plane * x.n + i, cnt);
  }
}

// Totals per plane: the sum of the plane's per-resource counts, once per call behind the last tile.  One wave per plane.
struct CrossTotalsArgs { const CBH_G u32* by_r; CBH_G u64* totals; u32 mr, bits; };   // `bits`: of a lane's largest sum
__global__ __launch_bounds__(64) void cbh_cross_review_totals_kernel(CrossTotalsArgs x) {
  const u32 lane = threadIdx.x & 63u;
  const CBH_G u32* c = x.by_r + (size_t)blockIdx.x * x.mr;
  u64 s = 0, total;
  for (u64 j = lane; j < x.mr; j += 64u) s += c[j];
  (void)cx_wave_prefix(s, x.bits, lane, total);
  if (lane == 0u) x.totals[blockIdx.x] = total;
}

// The pair list: the pairs of the call's range with a set bit in one of the chosen kind's SELECTED planes, in ascending bit index -
// ascending (pair_r, pair_p) -, with the bits of the pair in ALL of the kind's planes as its mask.  The order is part of the contract, so
// the list is an ordered compaction, not an append: per word the OR of the selected planes and its popcount, a sum per wave of 64
// words (count), one wave that turns the sums into offsets and carries the running base from tile to tile in device memory
// (scan: state[0] = pairs up to and including this tile, state[1] = pairs before it), and the scatter, which writes
// (q % n, r0 + q / n, mask) at base + rank while that is below the cap.  state[0] after the last tile is the number of pairs.
struct CrossPairArgs {
  const CBH_G u64* planes;   // [a][words]: the chosen kind's planes of the tile
  CBH_G u32* wavesum;        // [(words + 63) / 64]: pairs per 64 words; after the scan their exclusive offsets within the tile
  CBH_G u64* state;          // [2]
  CBH_G u32* pair_p; CBH_G u32* pair_r; CBH_G u64* pair_mask;   // [cap]
  u64 sel, cap;              // bit k of `sel` = plane k takes part
  u32 n, a, words, r0;       // `r0`: the tile's first resource
};
__device__ __forceinline__ u64 cx_pair_word(const CrossPairArgs& x, u32 w) {
  u64 m = 0;
  for (u32 k = 0; k < x.a; ++k) if ((x.sel >> k) & 1ull) m |= x.planes[(size_t)k * x.words + w];
  return m;
}
__global__ __launch_bounds__(256) void cbh_cross_review_pair_count_kernel(CrossPairArgs x) {
  const u64 w64 = (u64)blockIdx.x * 256u + threadIdx.x;
  const u32 lane = threadIdx.x & 63u;
  const bool live = w64 < x.words;
  const u32 c = live ? (u32)__builtin_popcountll(cx_pair_word(x, (u32)w64)) : 0u;
  u64 total;
  (void)cx_wave_prefix(c, 7u, lane, total);
  if (lane == 0u && live) x.wavesum[w64 >> 6] = (u32)total;
}
__global__ __launch_bounds__(64) void cbh_cross_review_pair_scan_kernel(CrossPairArgs x) {
  const u32 lane = threadIdx.x & 63u;
  const u32 nw = (x.words + 63u) / 64u, per = (nw + 63u) / 64u;
  const u32 lo = lane * per < nw ? lane * per : nw, hi = lo + per < nw ? lo + per : nw;
  u64 s = 0, total;
  for (u32 w = lo; w < hi; ++w) s += x.wavesum[w];
  u64 p = cx_wave_prefix(s, 33u, lane, total);   // (a tile has fewer than 2^32 pairs)
  for (u32 w = lo; w < hi; ++w) { const u32 c = x.wavesum[w]; x.wavesum[w] = (u32)p; p += c; }
  if (lane == 0u) { const u64 before = x.state[0]; x.state[1] = before; x.state[0] = before + total; }
}
__global__ __launch_bounds__(256) void cbh_cross_review_pair_scatter_kernel(CrossPairArgs x) {
  const u64 w64 = (u64)blockIdx.x * 256u + threadIdx.x;
  const u32 lane = threadIdx.x & 63u;
  const bool live = w64 < x.words;
  const u32 w = (u32)w64;
  u64 m = live ? cx_pair_word(x, w) : 0ull;
  u64 total;
  const u64 pre = cx_wave_prefix((u32)__builtin_popcountll(m), 7u, lane, total);
  if (!m) return;   // (behind the last ballot)
  u64 rank = x.state[1] + x.wavesum[w >> 6] + pre;
  while (m && rank < x.cap) {
    const u32 b = (u32)__builtin_ctzll(m);
    m &= m - 1ull;
    const u32 q = w * 64u + b;   // (below n * mt < 2^32)
    u64 mask = 0;
    for (u32 k = 0; k < x.a; ++k) mask |= ((x.planes[(size_t)k * x.words + w] >> b) & 1ull) << k;   // (all of the pair's, selected or not)
    x.pair_p[rank] = q % x.n; x.pair_r[rank] = x.r0 + q / x.n; x.pair_mask[rank] = mask;
    ++rank;
  }
}
