// Cross-product batches built on the device (cerbos_hip.h cbh_batch_upload_cross) and the allow bitmap of a resident batch
// (cbh_result_download_allow_bits).  Three small kernels, none of them on the decision path: the product they build is an ordinary
// resident batch the decision kernels read unchanged.  And the two kernels of the DIRECT road (cbh_cross_upload_ex) - the one lane that
// writes the action words, and the gather that turns chosen pairs of a set into a resident batch (cbh_cross_pairs_upload) -, which
// materialises no product: its decision kernels are the flat kernels' CROSS instantiations (cbh_check_flat.h), which read the
// halves' compact form in place and write ballots.  And the lane per principal that writes a wide set's role words.
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
