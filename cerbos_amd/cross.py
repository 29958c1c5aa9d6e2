"""Cross-product batches: N principals x M resources x A actions decided from N + M flattened messages.

Bulk questions - "which of these users may do what to which of these documents" (audits, what-if runs over a
stored population) - are a cross product, and flattening N*M CheckInputs would spend nearly all of the time
re-parsing the same N principals and M resources (the engine is ingest bound end to end).  Here
the two halves are flattened ONCE each, in a single flattener call so that they share one batch-local string
table and one heap, and the N*M device requests are laid out with vectorised gathers: principal-side fields and
columns tile, resource-side ones repeat.  Every request carries the same actions.  The result is an ordinary
``flatten.Batch`` (``cbh_batch``), so the kernels and the resident path are unchanged.

Routing order comes for free: the kernels like requests ordered by (kind, resource version, resource scope, role
list) - here the M resources are ordered by route, the N principals by role list, and the product is laid out
resource-major: requests are then ordered by route, and by role list within every resource (all a wave needs:
its 64 lanes share the policy buckets and walk them equally often); no N*M-element sort is needed.  Device request q = j' * N + i' pairs the
j'-th resource and the i'-th principal of those orders; ``effect_cube`` maps results back to [i][j][action].
"""
from __future__ import annotations

import numpy as np

from .flatten import (RQ_ACT_CNT, RQ_ACT_OFF, RQ_KIND, RQ_NFIELDS, RQ_P_SCOPE, RQ_P_VERSION, RQ_PRINCIPAL_ID, RQ_R_SCOPE,
                      RQ_R_VERSION, RQ_ROLE_CNT, RQ_ROLE_OFF, RQ_S_KIND, RQ_S_P_SCOPE, RQ_S_P_VERSION, RQ_S_R_SCOPE,
                      RQ_S_R_VERSION, RQ_S_RESOURCE_ID, Batch)

P_FIELDS = (RQ_PRINCIPAL_ID, RQ_P_SCOPE, RQ_P_VERSION, RQ_ROLE_OFF, RQ_ROLE_CNT, RQ_S_P_SCOPE, RQ_S_P_VERSION)
R_FIELDS = (RQ_KIND, RQ_R_SCOPE, RQ_R_VERSION, RQ_S_RESOURCE_ID, RQ_S_KIND, RQ_S_R_SCOPE, RQ_S_R_VERSION)


def cross_halves(flattener, principals, resources, actions, aux_data, default_policy_version, default_scope, sort):
    """The N + M halves flattened in one call (principals first; input 0 carries the actions) and the orders of the product:
    -> (halves batch, p_order, r_order, action ids)."""
    n, m, a = len(principals), len(resources), len(actions)
    if a > 64:
        raise ValueError("at most 64 actions per cross-product batch")
    aux = aux_data if isinstance(aux_data, (list, tuple)) else [aux_data] * n
    blank_p, blank_r = {"id": "", "roles": []}, {"kind": "", "id": ""}
    halves = [dict({"principal": p, "resource": blank_r, "actions": list(actions) if i == 0 else []},
                   **({"auxData": aux[i]} if aux[i] else {})) for i, p in enumerate(principals)]
    halves += [{"principal": blank_p, "resource": r, "actions": []} for r in resources]
    h = flattener.flatten(halves, default_policy_version, default_scope, sort=False)
    assert h.n_requests == n + m
    hp, hr = h.req_u32[:, :n], h.req_u32[:, n:]
    if sort and n * m > 1:
        # principals by (role count, order-sensitive role-list signature), resources by (kind, version, scope):
        # the keys of flatten.sort_batch_by_route, applied to the halves
        cnt = hp[RQ_ROLE_CNT].astype(np.int64)
        sig = np.zeros(n, dtype=np.uint64)
        with np.errstate(over="ignore"):
            for i in range(n):
                o, c = int(hp[RQ_ROLE_OFF, i]), int(cnt[i])
                k = np.arange(c, dtype=np.uint64)
                sig[i] = ((h.roles[o:o + c].astype(np.uint64) + np.uint64(1)) * (k * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0xC2B2AE3D27D4EB4F))).sum(dtype=np.uint64)
        p_order = np.lexsort((sig, cnt))
        r_order = np.lexsort((hr[RQ_R_SCOPE], hr[RQ_R_VERSION], hr[RQ_KIND]))
    else:
        p_order, r_order = np.arange(n), np.arange(m)
    act_ids = h.tuple_action[:a] if a else np.zeros(0, dtype=np.uint32)     # input 0 carried the actions
    return h, p_order, r_order, act_ids


def cross_product_batch(flattener, columns, principals, resources, actions, aux_data=None,
                        default_policy_version="default", default_scope="", sort=True) -> Batch:
    """``flattener``: ``flatten.Flattener`` or ``ingest.WireFlattener``; ``columns``: ``LoweredTable.columns``.
    ``aux_data`` (one dict, or one per principal) is visible to every request of that principal."""
    n, m, a = len(principals), len(resources), len(actions)
    h, p_order, r_order, act_ids = cross_halves(flattener, principals, resources, actions, aux_data, default_policy_version, default_scope, sort)
    nm = n * m
    hp, hr = h.req_u32[:, :n], h.req_u32[:, n:]
    b = Batch()
    b.n_requests, b.n_tuples, b.n_strings = nm, nm * a, h.n_strings
    req = np.zeros((RQ_NFIELDS, nm), dtype=np.uint32)
    for f in P_FIELDS:
        req[f] = np.tile(hp[f, p_order], m)
    for f in R_FIELDS:
        req[f] = np.repeat(hr[f, r_order], n)
    req[RQ_ACT_OFF] = np.arange(nm, dtype=np.uint32) * a
    req[RQ_ACT_CNT] = a
    b.req_u32 = req
    ncol = len(columns)
    b.col_tag = np.empty((ncol, nm), dtype=np.uint8)
    b.col_val = np.empty((ncol, nm), dtype=np.uint64)
    for c, (root, _) in enumerate(columns):
        if root == "R":
            b.col_tag[c], b.col_val[c] = np.repeat(h.col_tag[c, n:][r_order], n), np.repeat(h.col_val[c, n:][r_order], n)
        else:       # principal attributes and auxiliary data travel with the principal
            b.col_tag[c], b.col_val[c] = np.tile(h.col_tag[c, :n][p_order], m), np.tile(h.col_val[c, :n][p_order], m)
    b.tuple_action = np.tile(act_ids, nm).astype(np.uint32)
    b.tuple_req = np.repeat(np.arange(nm, dtype=np.uint32), a)
    b.roles, b.heap_tag, b.heap_val = h.roles, h.heap_tag, h.heap_val
    b.str_off, b.str_bytes, b.str_flags = h.str_off, h.str_bytes, h.str_flags
    b.vreq_input = np.arange(nm, dtype=np.int64)
    b.actions_per_request = None        # nm lists would defeat the purpose: read results through the cubes below
    b.shape = (n, m, a)
    b.p_order, b.r_order = p_order, r_order
    return b


def cross_product_upload(table, flattener, columns, principals, resources, actions, aux_data=None,
                         default_policy_version="default", default_scope="", sort=True, device_index=0):
    """The same product built ON THE DEVICE (``capi.Table.upload_cross``): only the N + M halves cross the host link.  Returns the
    resident batch (``capi.DeviceBatch``) with ``shape``, ``p_order``, ``r_order``, so ``effect_cube`` / ``result_cubes`` /
    ``allow_cube`` accept it.  ``columns`` is accepted for symmetry with ``cross_product_batch``: which half a column comes from
    is read off the table image."""
    h, p_order, r_order, act_ids = cross_halves(flattener, principals, resources, actions, aux_data, default_policy_version, default_scope, sort)
    return upload_halves(table, h, len(principals), len(resources), act_ids, p_order, r_order, device_index)


def upload_halves(table, halves, n, m, act_ids, p_order, r_order, device_index=0):
    """``cross_product_upload`` for halves that are flattened already (a caller who keeps them across policy changes);
    an order of None is the identity."""
    db = table.upload_cross(halves, n, m, act_ids, p_order, r_order, device_index=device_index)
    db.shape = (n, m, len(act_ids))
    db.p_order = np.arange(n) if p_order is None else np.asarray(p_order)
    db.r_order = np.arange(m) if r_order is None else np.asarray(r_order)
    return db


def cross_direct_upload(table, flattener, columns, principals, resources, actions, aux_data=None,
                        default_policy_version="default", default_scope="", sort=True, device_index=0, accept=0):
    """``cross_product_upload`` without the product (``capi.Table.cross_upload``): the device keeps the N + M halves and
    ``capi.CrossSet.check`` decides tiles of resources straight from them - N * M is bounded by what the caller wants back, not by
    device memory.  Returns the ``capi.CrossSet`` with ``shape``, ``p_order``, ``r_order`` (``allow_cube_planes`` accepts it), or
    None where the set has no direct form: take ``cross_product_upload``, which gives the same answers.  ``accept``:
    ``capi.CX_DERIVED_ROLES`` | ``capi.CX_ACTION_GROUPS`` | ``capi.CX_ROLE_GROUPS`` - tables with derived roles, more than four
    actions, principals with five to sixteen roles (decided four roles at a time; ``sort=True`` orders the principals by role
    count, which keeps the wide ones together in a wave); by default none."""
    h, p_order, r_order, act_ids = cross_halves(flattener, principals, resources, actions, aux_data, default_policy_version, default_scope, sort)
    return direct_upload_halves(table, h, len(principals), len(resources), act_ids, p_order, r_order, device_index, accept)


def direct_upload_halves(table, halves, n, m, act_ids, p_order, r_order, device_index=0, accept=0):
    """``cross_direct_upload`` for halves that are flattened already; an order of None is the identity.  ``accept`` as there
    (``capi.CX_ROLE_GROUPS``: the halves may hold principals with up to sixteen roles)."""
    cs = table.cross_upload(halves, n, m, act_ids, p_order, r_order, device_index=device_index, accept=accept)
    if cs is not None:
        cs.p_order = np.arange(n) if p_order is None else np.asarray(p_order)
        cs.r_order = np.arange(m) if r_order is None else np.asarray(r_order)
    return cs


def allow_cube_planes(cross_set, r_begin, r_end, planes):
    """Planes of ``capi.CrossSet.check(r_begin, r_end)`` (``allow`` or ``flagged``: uint64[a][words]) -> bool[n][r_end - r_begin][a]
    in the CALLER's orders: [i][j][k] = principals[i], the j-th of the tile's resources taken in the caller's resource order (the
    tile holds resources ``r_order[r_begin:r_end]``), actions[k]."""
    n, _, a = cross_set.shape
    mt = r_end - r_begin
    by = np.ascontiguousarray(planes, dtype="<u8").view(np.uint8).reshape(a, -1)
    dev = np.unpackbits(by, axis=1, count=n * mt, bitorder="little").astype(bool).reshape(a, mt, n)   # [k][j'][i']
    res = np.asarray(cross_set.r_order)[r_begin:r_end]
    out = np.empty((n, mt, a), dtype=bool)
    out[np.ix_(cross_set.p_order, np.argsort(np.argsort(res)))] = dev.transpose(2, 1, 0)
    return out


def flagged_pairs(cross_set, r_begin, r_end, flagged):
    """``flagged`` planes of ``capi.CrossSet.check(r_begin, r_end, want_flagged=True)`` -> (pair_p, pair_r, action_mask): the pairs of
    the tile with a flagged action, in DEVICE order (ascending bit index: resource-major) - ``pair_r = r_begin + q // n``,
    ``pair_p = q % n``, what ``capi.CrossSet.pairs_batch`` takes - and per pair a uint64 with bit k set = action k is flagged."""
    n, _, a = cross_set.shape
    nt = n * (r_end - r_begin)
    by = np.ascontiguousarray(flagged, dtype="<u8").view(np.uint8).reshape(a, -1)
    bits = np.unpackbits(by, axis=1, count=nt, bitorder="little").astype(bool)          # [k][q]
    q = np.flatnonzero(bits.any(axis=0))
    mask = np.zeros(q.size, dtype=np.uint64)
    for k in range(a):
        mask |= bits[k, q].astype(np.uint64) << np.uint64(k)
    return (q % n).astype(np.uint32), (r_begin + q // n).astype(np.uint32), mask


def review_counts(cross_set, r_begin, r_end, result):
    """``capi.CrossSet.review(r_begin, r_end, ...)`` -> the same in the CALLER's orders, as ``allow_cube_planes`` gives cubes: a
    namespace with ``allow_by_principal`` / ``flagged_by_principal`` uint32[n][a] - row i = principals[i] -, ``allow_by_resource`` /
    ``flagged_by_resource`` uint32[r_end - r_begin][a] - row j = the j-th of the tile's resources taken in the caller's resource
    order (the tile holds resources ``r_order[r_begin:r_end]``) -, ``totals`` as they are, and the pairs as (``pair_p``, ``pair_r``)
    = indices into the caller's principals and resources, in the list's order, with ``pair_mask`` and ``n_pairs``.  What the review
    did not return stays None."""
    from types import SimpleNamespace
    po, ro = np.asarray(cross_set.p_order), np.asarray(cross_set.r_order)
    rank = np.argsort(np.argsort(ro[r_begin:r_end]))          # device position within the tile -> place in the caller's order

    def by_principal(x):
        if x is None:
            return None
        out = np.empty((x.shape[1], x.shape[0]), dtype=x.dtype)
        out[po] = x.T
        return out

    def by_resource(x):
        if x is None:
            return None
        out = np.empty((x.shape[1], x.shape[0]), dtype=x.dtype)
        out[rank] = x.T
        return out

    return SimpleNamespace(
        allow_by_principal=by_principal(result.allow_by_principal), flagged_by_principal=by_principal(result.flagged_by_principal),
        allow_by_resource=by_resource(result.allow_by_resource), flagged_by_resource=by_resource(result.flagged_by_resource),
        totals=result.totals, n_pairs=result.n_pairs, pair_mask=result.pair_mask,
        pair_p=None if result.pair_p is None else po[result.pair_p], pair_r=None if result.pair_r is None else ro[result.pair_r])


def allow_cube(batch, bits):
    """``capi.Table.download_allow_bits`` of the batch -> bool[n][m][a]: [i][j][k] = principals[i] may actions[k] on resources[j]."""
    n, m, a = batch.shape
    allowed = np.unpackbits(np.ascontiguousarray(bits, dtype="<u8").view(np.uint8), count=n * m * a, bitorder="little").astype(bool)
    return _cube(batch, allowed)


def _cube(batch, per_tuple):
    n, m, a = batch.shape
    out = np.empty((n, m, a), dtype=per_tuple.dtype)
    out[np.ix_(batch.p_order, batch.r_order)] = np.asarray(per_tuple).reshape(m, n, a).transpose(1, 0, 2)
    return out


def effect_cube(batch, res):
    """``capi.Result`` of the batch -> uint8[n][m][a] of CBH_EFFECT_*: [i][j][k] = principals[i], resources[j], actions[k]."""
    return _cube(batch, res.effect)


def result_cubes(batch, res):
    """All per-action outputs as [n][m][a] cubes, and the derived-role masks as [n][m]."""
    n, m, _ = batch.shape
    edr = None
    if res.edr is not None:
        edr = np.empty((n, m), dtype=np.uint64)
        edr[np.ix_(batch.p_order, batch.r_order)] = np.asarray(res.edr).reshape(m, n).T
    return {f: (_cube(batch, getattr(res, f)) if getattr(res, f) is not None else None) for f in ("effect", "policy", "scope", "status")}, edr
