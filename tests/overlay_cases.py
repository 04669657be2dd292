"""Cases for the genesis-delegate branch of the ledger-view checks on overlay
slots (tests/test_overlay_rule.py, test_gpu_overlay.py): view schedules with
genesis delegations, seeded header rows that reach every outcome of the branch,
and a signed, linked chain that pools and genesis delegates forge together
under d = 1/2.  Keys and rows come from the helpers of ledger_cases.py;
expectations come from ledger.rule / fold_rule with ``genesis`` (hashlib,
Fraction, a dict), never from the library."""
import functools

import numpy as np

import ledger_cases as LC
from ouroboros_network_amd import ledger as L

DEN63 = 2**63 - 25                       # d = 1 / DEN63: one overlay slot at s = 0, the next at s = DEN63
FAR = 2**63 + 5000                       # the last entry's first slot: s reaches 2^63 - 5001 there
ASC_INVS = (1, 20, 3)
# (first_slot, d, genesis keys, pools)
SHAPE = [(0, (1, 1), 5, 2), (1000, (1, 2), 7, 3), (2000, (3, 10), 1, 2), (3000, (0, 1), 0, 2),
         (4000, (1, DEN63), 7, 2), (FAR, (1, 2), 5, 3)]


@functools.lru_cache(maxsize=None)
def views():
    """(views, pool keys per entry, delegate keys per entry in GENESIS-ID order,
    {asc_inv: GenesisDelegs}): six entries with d = 1, 1/2, 3/10, 0, 1 / (2^63 -
    25) and 1/2, and 5, 7, 1, 0, 7, 5 genesis keys.  The seven delegates are the
    same keys in every entry; entry 1's first pool is also delegate 0."""
    rng = np.random.default_rng(9191)
    delegs = [LC.Key(rng) for _ in range(7)]
    gids = [rng.bytes(28) for _ in range(7)]
    entries, pkeys, dkeys, gens = [], [], [], []
    for j, (first, d, ngen, npool) in enumerate(SHAPE):
        ks = [LC.Key(rng) for _ in range(npool)]
        if j == 1:
            ks[0] = delegs[0]            # a delegate that is also a registered pool
        pkeys.append(ks)
        entries.append(L.Entry(first, d, tuple(k.pool(LC._sigma(rng)) for k in ks)))
        # another permutation of the delegates per entry, so that the delegates'
        # order differs from their genesis keys' order
        perm = [int(x) for x in rng.permutation(7)[:ngen]]
        pairs = sorted(((gids[i], delegs[p]) for i, p in enumerate(perm)), key=lambda t: t[0])
        dkeys.append([k for _, k in pairs])
        gens.append(tuple(L.GenDeleg(g, k.id, k.vrf_hash) for g, k in pairs))
    v = L.LedgerViews(entries)
    return v, pkeys, dkeys, {a: L.GenesisDelegs(gens, a) for a in ASC_INVS}


def classify(e, asc_inv, ngen, slot):
    """'pool' (not an overlay slot), 'inactive', or the scheduled index"""
    if not L.is_overlay_slot(e.first_slot, e.d, slot):
        return "pool"
    ix = L.classify_overlay_slot(e.first_slot, e.d, asc_inv, ngen, slot)
    return "inactive" if ix is None else ix


def _slots_of(j):
    """the slots a row of entry j may take: the entry's first 600, its last, and
    for the two long entries those around the largest s"""
    first = SHAPE[j][0]
    out = list(range(first, first + 600))
    if j == 4:   # s = DEN63 is the second (and last reachable) overlay slot of d = 1 / DEN63
        out += [first + DEN63 - 1, first + DEN63, first + DEN63 + 1, FAR - 1]
    elif j == 5:
        out += [2**64 - 1 - x for x in range(80)]
    else:
        out += [SHAPE[j + 1][0] - 1]
    return out


@functools.lru_cache(maxsize=None)
def rows(asc_inv):
    """~700 seeded rows under the schedule with this asc_inv: per row an entry,
    a slot class drawn first (so that active slots are as common under asc_inv =
    20 as under 1), an issuer (the scheduled delegate, another delegate, a pool
    of the entry, a stranger), the right or a wrong VRF key, a period inside or
    outside the certificate's bounds."""
    v, pkeys, dkeys, gens = views()
    rng = np.random.default_rng(1000 + asc_inv)
    stranger = LC.Key(rng)
    by_class = []
    for j, e in enumerate(v.entries):
        c = {"pool": [], "inactive": [], "active": []}
        for s in _slots_of(j):
            k = classify(e, asc_inv, len(dkeys[j]), s)
            c[k if isinstance(k, str) else "active"].append(s)
        by_class.append(c)
    out = []
    # the edges first: slot 0 of every entry, the slot below it, the largest slots
    for j, e in enumerate(v.entries):
        for slot in (e.first_slot, e.first_slot - 1, e.first_slot + 1):
            if slot >= 0:
                out.append((j if slot >= e.first_slot else j - 1, slot))
    out += [(4, 4000 + DEN63), (5, 2**64 - 1), (5, 2**64 - 2), (5, FAR)]
    while len(out) < 700:
        j = int(rng.integers(0, len(v.entries)))
        want = ("active", "active", "inactive", "pool")[int(rng.integers(0, 4))]
        pool = by_class[j][want]
        if pool:
            out.append((j, pool[int(rng.integers(0, len(pool)))]))
    res = []
    for j, slot in out:
        e = v.entries[j]
        cls = classify(e, asc_inv, len(dkeys[j]), slot)
        who = int(rng.integers(0, 8))
        if isinstance(cls, int) and who < 4:
            key = dkeys[j][cls]                                   # the scheduled delegate
        elif who < 6 and dkeys[j]:
            key = dkeys[j][int(rng.integers(0, len(dkeys[j])))]   # some delegate
        elif who < 7:
            key = pkeys[j][int(rng.integers(0, len(pkeys[j])))]   # a pool of the entry
        else:
            key = stranger
        vrf = key.vrf if rng.integers(0, 4) else stranger.vrf
        kp = slot // LC.SPKP
        c0 = (kp, kp, kp, max(kp - LC.MAX_EVO + 1, 0), kp + 1,
              max(kp - LC.MAX_EVO, 0) if kp >= LC.MAX_EVO else kp + 2)[int(rng.integers(0, 6))]
        res.append(LC._row(key.cold, vrf, slot, LC._beta(rng), c0, int(rng.integers(0, 4))))
    return res


def expect(v, g, rws, genesis):
    out = [L.rule(v, g, r[0], r[1], r[2], r[3], r[4], oracle=LC.OL, genesis=genesis) for r in rws]
    return np.array([b for b, _ in out], np.uint8), np.array([r for _, r in out], np.uint32)


@functools.lru_cache(maxsize=None)
def all_rows():
    """the ~2,100 rows of the three schedules, with (asc_inv, rows, bits, view rows)
    per schedule, the expected side computed once"""
    v, _, _, gens = views()
    out = []
    for a in ASC_INVS:
        r = rows(a)
        b, p = expect(v, LC.G_MAIN, r, gens[a])
        out.append((a, r, b, p))
    return out


def outcome(b):
    """the outcomes the issue names, of one row's expected bits"""
    b = int(b)
    o = []
    if not b & L.LV_OVERLAY:
        return ["not overlay"]
    if not b & L.LV_KES_PERIOD_OK:
        o.append("overlay, period out of bounds")
    if not b & L.LV_OVERLAY_ACTIVE:
        o.append("overlay, inactive")
    elif not b & L.LV_POOL_KNOWN:
        o.append("active, wrong cold key")
    elif not b & L.LV_VRF_KEY_OK:
        o.append("right cold key, wrong VRF key")
    else:
        o.append("active, right delegate")
    return o


OUTCOMES = ("not overlay", "overlay, inactive", "active, right delegate", "active, wrong cold key",
            "right cold key, wrong VRF key", "overlay, period out of bounds")


def table_for(v, genesis, known=None):
    """a counters table with a row for every pool and every delegate"""
    return L.Counters(sorted(set(v.all_pool_ids()) | set(genesis.all_delegate_ids())), known)


def views_k(k, ngen=7):
    """ledger_cases.views_k with d = 1/2 and the same ngen genesis keys per entry"""
    rng = np.random.default_rng(70 + k)
    ks = [LC.Key(rng), LC.Key(rng)]
    ds = [LC.Key(rng) for _ in range(ngen)]
    gids = sorted(rng.bytes(28) for _ in range(ngen))
    entries = [L.Entry(10 * j, (1, 2), tuple(x.pool((1 + j % 3, 3 + j % 5)) for x in ks))
               for j in range(k)]
    gen = tuple(L.GenDeleg(g, d.id, d.vrf_hash) for g, d in zip(gids, ds))
    return L.LedgerViews(entries), ks, ds, L.GenesisDelegs([gen] * k, 1)


# ---- a signed, linked chain of four pools and two genesis delegates ---------------------
N_TPRAOS = 40
CHAIN_ASC_INV = 2
DELEG = (5, 6)        # ledger_cases.pool_keys indices of the two delegates


@functools.lru_cache(maxsize=None)
def chain_stream():
    """ledger_cases.chain_stream's construction under d = 1/2 in all three view
    entries, asc_inv = 2 and two genesis keys: 250 Byron headers (chunk 0 of 256
    is mixed), then 40 TPraos headers whose slots are picked class by class --
    pools forge the non-overlay slots, the scheduled delegate the active overlay
    slots.  Header 3 sits on an inactive overlay slot, header 9 comes from the
    wrong delegate, header 12 from a pool on an active overlay slot; delegate
    0's counter falls across the chunk boundary (headers 255 -> 256 of the
    stream are both its) and delegate 1's inside chunk 1."""
    import envelope_cases as EC
    from ouroboros_network_amd import envelope as E
    from ouroboros_network_amd import header as H
    from ouroboros_network_amd.tpraos import EpochNonces

    byron = EC.good_chain(LC.N_BYRON, 0, ebb_every=9, extra_step=11)
    last = E.header_record(byron[-1], EC.VAL_CFG)
    base = last.slot + 1
    first = [0, base + 100, base + 250]
    eta = [None, b"\x33" * 32, b"\x77" * 32]
    entry_of = lambda s: max(j for j, f in enumerate(first) if f <= s)  # noqa: E731
    ids = []
    for i in range(7):
        cold_pk, _, vrf_pk, _ = LC.pool_keys(i)
        ids.append((L.pool_id(cold_pk), L.vrf_key_hash(vrf_pk)))
    pools = tuple(L.Pool(ids[i][0], ids[i][1], (1, 1)) for i in range(4))
    views_ = L.LedgerViews([L.Entry(f, (1, 2), pools) for f in first])
    gid = sorted([b"\x11" * 28, b"\x99" * 28])
    gen = tuple(L.GenDeleg(gid[x], ids[DELEG[x]][0], ids[DELEG[x]][1]) for x in range(2))
    genesis = L.GenesisDelegs([gen] * 3, CHAIN_ASC_INV)

    def cls(s):
        return classify(views_.entries[entry_of(s)], CHAIN_ASC_INV, 2, s)

    # per header: the class its slot must have (an int: active with that
    # delegate scheduled) and who forges it (None: whoever is scheduled)
    plan = []
    for i in range(N_TPRAOS):
        plan.append(("pool", i % 4) if i % 2 == 0 else (len(plan) // 2 % 2, None))
    plan[3] = ("inactive", DELEG[0])
    plan[5], plan[6] = (0, None), (0, None)          # stream headers 255 and 256: delegate 0
    plan[9] = (1, DELEG[0])                          # the wrong delegate
    plan[12] = (0, 2)                                # a pool on an active overlay slot
    plan[20] = (1, None)
    slots, pool_of, s = [], [], base
    for i, (want, who) in enumerate(plan):
        s += 6 + (17 if i % 13 == 12 else 0)         # (gaps, to cross all three entries)
        while cls(s) != want:
            s += 1
        slots.append(s)
        pool_of.append(DELEG[want] if who is None else who)
    counters = [10 + i // 8 for i in range(N_TPRAOS)]
    counters[5], counters[6] = 10, 8                 # delegate 0 falls across the chunk boundary
    counters[20] = 3                                 # delegate 1 falls inside chunk 1
    nonce_of = lambda s: eta[entry_of(s)]            # noqa: E731
    tp, _ = LC.signed_chain4(last.hash, slots, last.block_no + 1, [nonce_of(s) for s in slots],
                             pool_of, counters)
    rws = []
    for r in tp:
        h = H.parse_header(r)
        rws.append(LC._row(h.issuer_vk, h.vrf_vk, h.slot, h.leader_output, h.ocert_kes_period,
                           h.ocert_counter))
    known = {ids[0][0]: 10, ids[DELEG[1]][0]: 7}     # the others: in the table, no counter yet
    return dict(raws=byron + tp, n_byron=len(byron),
                epochs=EpochNonces(first_slot=first, nonce=[n or bytes(32) for n in eta],
                                   neutral=[n is None for n in eta]),
                views=views_, genesis=genesis, rows=rws, known=known, plan=plan,
                table_ids=[i[0] for i in ids[:4]] + [ids[DELEG[0]][0], ids[DELEG[1]][0]])


def chain_expect(s, genesis=True):
    """(ledger, pool_row, counters after) of the whole stream, in Python"""
    gen = s["genesis"] if genesis else None
    bits, prow = expect(s["views"], LC.G_CHAIN, s["rows"], gen)
    bits, known = L.fold_rule(s["views"], bits, prow, [r[5] for r in s["rows"]], s["known"],
                              genesis=gen)
    nb = s["n_byron"]
    return (np.concatenate([np.zeros(nb, np.uint8), bits]),
            np.concatenate([np.full(nb, L.LV_NO_POOL, np.uint32), prow]), known)
