"""The Byron transaction-witness rule (byron_witness.py), stated in Python: the
witness vector's shape pinned by the reference's golden Byron block, the signed
message's bytes, and the rule on the case set -- that every case is what its
builder meant it to be.  CPU only; no library entry is called."""
import hashlib

import numpy as np

import byron_block_cases as C
import byron_witness_cases as WC
import oracle_ffi as O
from ouroboros_network_amd import byron_witness as BW


def test_golden_block_pins_the_witness_vector_shape():
    """payload[707:847] of the on-disk block is 81 82 00 d8 18 58 85 82 58 40
    <64> 58 40 <64>: one tx row, one kind-0 row, its XPub, the oracle's verdict
    (the key is an ASCII placeholder, so it does not verify) -- in both forms."""
    disk = C.golden()["cardano_disk_Byron_regular"]
    vec = disk[707:847]
    assert vec[:10].hex() == "818200d8185885825840" and vec[74:76].hex() == "5840"
    assert WC.GOLDEN_MAGIC == C.parts()["magic_value"]
    for name in ("cardano_disk_Byron_regular", "cardano_n2n_Byron_regular"):
        raw = C.golden()[name]
        assert raw.count(vec) == 1
        b = BW.parse_byron_witnesses(raw)
        assert len(b.tx_spans) == 1 and len(b.witnesses) == 1 and b.magic == WC.GOLDEN_MAGIC
        w = b.witnesses[0]
        assert (w.tx, w.kind, w.key, w.sig) == (0, 0, vec[10:74], vec[76:140])
        assert raw[b.tx_spans[0][0] + b.tx_spans[0][1]:][:140] == vec
        tx_id = hashlib.blake2b(raw[b.tx_spans[0][0]:][:b.tx_spans[0][1]], digest_size=32).digest()
        ok = O.ed25519_verify_byron(w.sig, BW.byron_witness_message(b.magic, 0, tx_id), w.key[:32])
        st, verdict, n_bad, ids, rows = WC.expect(raw, WC.GOLDEN_MAGIC)
        assert (st, ids, rows) == (BW.PACK_OK, [tx_id], [(0, 0, w.key, ok)])
        assert (verdict, n_bad) == ((BW.BYW_ALL_OK, 0) if ok else (0, 1))
    assert BW.byron_witness_rule(C.golden()["cardano_disk_Byron_EBB"], 7, None)[:3] == (
        BW.PACK_EBB, BW.BYW_ALL_OK, 0)
    assert BW.byron_witness_status(C.golden()["cardano_disk_Mary"]) == BW.PACK_ESHELLEY


def test_message_bytes():
    tx_id = bytes(range(32))
    m = BW.byron_witness_message(WC.MAINNET_MAGIC, 0, tx_id)
    assert m.hex() == "011a2d964a095820" + tx_id.hex()
    assert BW.byron_witness_message(WC.MAINNET_MAGIC, 2, tx_id)[:8].hex() == "021a2d964a095820"
    want = {0: "00", 23: "17", 24: "1818", 255: "18ff", 256: "190100", 65535: "19ffff",
            65536: "1a00010000", 2**32 - 1: "1affffffff"}
    for magic, enc in want.items():
        for kind, tag in ((0, "01"), (2, "02")):
            assert BW.byron_witness_message(magic, kind, tx_id).hex() == tag + enc + "5820" + tx_id.hex()
    assert sorted({len(BW.byron_witness_message(m, 0, tx_id)) for m in WC.MAGICS}) == [36, 37, 38, 40]


def test_the_case_set_is_what_its_builders_meant():
    cs = WC.case_set()
    by_kind = {}
    for i, k in enumerate(cs["kinds"]):
        by_kind.setdefault(k, []).append(i)
    ok = lambda i: cs["status"][i] == BW.PACK_OK and cs["verdict"][i] == BW.BYW_ALL_OK  # noqa: E731
    # the valid families: every row verifies, the counts are the builders'
    for k in ("per_tx", "per_block", "span"):
        assert all(ok(i) for i in by_kind[k]), k
    per_tx = sorted(int(cs["nwit"][i]) for i in by_kind["per_tx"])
    assert per_tx == sorted([3 * c for c in WC.PER_TX[:-1]] * 2 + [256] * 2)
    assert [int(cs["ntx"][i]) for i in by_kind["per_block"]] == WC.TX_PER_BLOCK
    assert len(by_kind["span"]) == 4 * len(WC.TX_LENGTHS)
    for j, i in enumerate(by_kind["span"]):
        t = BW.parse_byron_witnesses(cs["raws"][i]).tx_spans[0]
        assert t[1] == WC.TX_LENGTHS[j // 4] and (int(cs["triple"][1][i]) + t[0]) % 4 == j % 4
    kinds_seen = {int(k) for k in cs["wit_kind"]}
    assert kinds_seen == {0, 2}
    # the golden blocks
    assert sorted(int(cs["status"][i]) for i in by_kind["golden_byron"]) == [0, 0, 6, 6]
    assert {int(cs["status"][i]) for i in by_kind["golden_shelley"]} == {BW.PACK_ESHAPE,
                                                                        BW.PACK_ESHELLEY}
    # one thing broken: the status, or exactly the rows the builder broke
    for kind, want in WC.BROKEN.items():
        (i,) = by_kind[kind]
        if isinstance(want, int):
            assert cs["status"][i] == want and cs["verdict"][i] == 0 and cs["nwit"][i] == 0, kind
            continue
        w0 = int(cs["wit_begin"][i])
        bad = [r for r in range(9) if not cs["wit_ok"][w0 + r]]
        assert cs["status"][i] == BW.PACK_OK and bad == want and cs["n_bad"][i] == len(want), kind
        assert cs["verdict"][i] == 0
    # the adversarial block: the oracle accepts some and rejects some, of both kinds
    (i,) = by_kind["adversarial"]
    w0, w1 = int(cs["wit_begin"][i]), int(cs["wit_begin"][i + 1])
    for kind in (0, 2):
        got = cs["wit_ok"][w0:w1][cs["wit_kind"][w0:w1] == kind]
        assert got[0] == 1 and 1 < got.sum() < got.size, kind
    # only blocks that slice give a verdict; rows number a few thousand at most
    assert not ((cs["verdict"] != 0) & ~np.isin(cs["status"], (BW.PACK_OK, BW.PACK_EBB))).any()
    assert 1000 < int(cs["wit_begin"][-1]) < 4000


def test_magics_and_the_headers_own_field():
    raws = WC.magic_set()
    own = WC.expected_arrays(raws, "header")
    # under each header's own field every block verifies but the last, whose
    # witnesses were signed under another magic than its header says: all fail
    assert own["verdict"].tolist() == [1] * len(WC.MAGICS) + [0]
    assert own["n_bad"].tolist() == [0] * len(WC.MAGICS) + [5]
    for k, m in enumerate(WC.MAGICS):
        v = WC.expected_arrays(raws, m)["verdict"].tolist()
        assert v == [1 if j == k else 0 for j in range(len(WC.MAGICS))] + [int(m == WC.GOLDEN_MAGIC)]
    assert {BW.parse_byron_witnesses(r).magic for r in raws[:-1]} == set(WC.MAGICS)


def test_first_offending_item_in_byte_order():
    """A shape error in an earlier witness vector comes before malformed CBOR
    later in the block; inside one element the outer walk's error comes first."""
    cs = WC.case_set()
    raw = cs["raws"][cs["kinds"].index("type_1")]
    assert BW.byron_witness_status(raw) == BW.PACK_ESHAPE
    assert BW.byron_witness_status(raw[:-1]) == BW.PACK_ESHAPE       # (the extra data cut short)
    good = cs["raws"][cs["kinds"].index("sig_bit")]
    assert BW.byron_witness_status(good[:-1]) == BW.PACK_ECBOR
    # a reserved head (0x1c) as the type of the witness after the unknown type,
    # inside the same element: the outer walk meets it before the vector is read
    key = WC.keypair(0, 55)[0]                  # witness (1, 2): 82 00 d8 18 58 85 82 58 40 <key>
    at = raw.index(key) - 8
    assert raw[at - 1:at + 3].hex() == "8200d818"
    bad = raw[:at] + b"\x1c" + raw[at + 1:]
    assert BW.byron_witness_status(bad) == BW.PACK_ECBOR
    # ... and as a well-formed 3 it is just the second unknown type
    assert BW.byron_witness_status(raw[:at] + b"\x03" + raw[at + 1:]) == BW.PACK_ESHAPE


def test_existing_kernels_resource_listing_is_the_parents():
    """profiles/byron_witnesses: the new listing without the new unit's lines is
    the parent's, line for line (no existing kernel is built differently)."""
    import os

    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                     "byron_witnesses")
    with open(os.path.join(d, "resources_parent.txt")) as f:
        parent = f.read().splitlines()
    with open(os.path.join(d, "resources_new.txt")) as f:
        new = f.read().splitlines()
    added = [ln for ln in new if ln.startswith(("csrc/kernels_byron_witness.hip:",
                                                "csrc/scan_excl.h:"))]
    assert [ln for ln in new if ln not in set(added)] == parent and len(parent) > 400
    names = [ln for ln in added if "Function Name" in ln]
    assert len(names) == 9 and sum("k_byron_witness_" in ln for ln in names) == 6
