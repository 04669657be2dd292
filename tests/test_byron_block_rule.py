"""The Byron block rule as byron_block.py states it (CPU): the reference's golden
Byron block pins the leaf form, the witnesses list form and the two payload
hashes; the golden EBB; the level-by-level root against the recursive
definition; and the statuses and bits of the blocks tests/byron_block_cases.py
builds."""
import hashlib

import pytest

import byron_block_cases as C
import oracle_ffi as O
from ouroboros_network_amd import byron as BY
from ouroboros_network_amd import byron_block as BB


def h(m):
    return hashlib.blake2b(m, digest_size=32).digest()


def test_golden_block_reproduces_all_four_header_hashes():
    """The pin.  Offsets into the tag-24 payload of the reference's
    CardanoNodeToNodeVersion1/Block_Byron_regular, found by the slicer and
    restated here as numbers."""
    wire = C.golden()["cardano_n2n_Byron_regular"]
    assert wire[:4] == b"\xd8\x18\x59\x03"
    payload = wire[5:]
    assert payload == C.golden()["cardano_disk_Byron_regular"]
    b = BB.parse_byron_block(payload)
    assert b.txs == [(612, 95)] and b.wits == [(707, 140)]
    assert b.dlg == (854, 2) and b.upd == (856, 4) and b.tx_num == 1
    assert payload[854:856] == b"\x9f\xff"
    root, wit, dlg, upd = b.claimed
    assert h(b"\x00" + payload[612:707]) == root
    assert h(b"\x9f" + payload[707:847] + b"\xff") == wit
    assert h(payload[854:856]) == dlg
    assert h(payload[856:860]) == upd
    assert b.proof(payload) == b.claimed
    magic = C.parts()["magic_value"]
    for raw in (wire, payload):
        assert C.expect(raw, magic) == (BB.PACK_OK, BB.BYB_ALL_OK, root)
        assert C.expect(raw, BY.HEADER_MAGIC) == (BB.PACK_OK, BB.BYB_ALL_OK, root)
        # another network: the signature and the magic field both fail, the body holds
        assert C.expect(raw, magic + 1)[1] == BB.BYB_ALL_OK & ~BB.BYB_HDR_OK
    assert O.ed25519_verify_byron(b.sig, b.message(magic), b.delegate_xpub[:32])


def test_golden_ebb():
    for name in ("cardano_disk_Byron_EBB", "cardano_n2n_Byron_EBB"):
        raw = C.golden()[name]
        assert BB.parse_byron_block(raw) is None
        assert C.expect(raw, 7) == (BB.PACK_EBB, BB.BYB_ALL_OK, bytes(32))
        assert BB.byron_block_counts(raw, 7) == (BB.PACK_EBB, 0, 0, 0)
        assert BB.byron_block_status(raw + b"\x00") == BB.PACK_ECBOR
        assert BB.byron_block_status(raw[:-1]) == BB.PACK_ECBOR


def test_level_by_level_root_equals_the_recursive_definition():
    leaves = [h(bytes([k & 255, k >> 8])) for k in range(301)]
    assert BB.merkle_root([]) == h(b"") == BB.merkle_root_levels([])
    assert BB.merkle_root(leaves[:1]) == leaves[0]
    assert BB.merkle_root(leaves[:3]) == h(b"\x01" + h(b"\x01" + leaves[0] + leaves[1]) + leaves[2])
    for n in range(301):
        assert BB.merkle_root_levels(leaves[:n]) == BB.merkle_root(leaves[:n]), n


def test_built_blocks_statuses_and_bits():
    cs = C.case_set()
    seen = set()
    for kind, raw, st, v in zip(cs["kinds"], cs["raws"], cs["status"], cs["verdict"]):
        seen.add(kind)
        if kind in ("count", "span"):
            assert (st, v) == (BB.PACK_OK, BB.BYB_ALL_OK), kind
        elif kind in C.BROKEN:
            assert st == BB.PACK_OK and v == C.must_be(kind), (kind, v)
        elif kind == "golden_shelley":
            # [tag >= 2, block] and its wire form; the bare Shelley forms are no [tag, block]
            assert (st, v) in ((BB.PACK_ESHELLEY, 0), (BB.PACK_ESHAPE, 0))
        else:
            assert kind == "golden_byron" and v == BB.BYB_ALL_OK and st in (BB.PACK_OK, BB.PACK_EBB)
    assert seen == {"count", "span", "golden_shelley", "golden_byron"} | set(C.BROKEN)
    assert (cs["status"] == BB.PACK_ESHELLEY).sum() == 6
    assert sorted(cs["ntx"][:len(C.TX_COUNTS)].tolist()) == C.TX_COUNTS
    # every span length at every alignment of the buffer
    buf, off, ln = cs["triple"]
    got = set()
    for kind, raw, o in zip(cs["kinds"], cs["raws"], off):
        if kind == "span":
            t = BB.parse_byron_block(raw).txs[0]
            got.add((t[1], (int(o) + t[0]) % 4))
    assert got == {(n, a) for n in C.TX_LENGTHS for a in range(4)}


@pytest.mark.parametrize("what", ["array3", "indef_block", "body3", "elem3", "tx_not_array",
                                  "proof_size", "trailing", "no_break"])
def test_shape_statuses(what):
    import numpy as np

    rng = np.random.default_rng(3)
    good = C.make_block(C.pairs_of(2, rng), form=0, indefinite=(what == "no_break"))
    b = BB.parse_byron_block(good)
    if what == "array3":
        assert good[:3] == b"\x82\x01\x83"
        raw, want = good[:2] + b"\x84" + good[3:], BB.PACK_ESHAPE
    elif what == "indef_block":
        raw, want = good[:2] + b"\x9f" + good[3:] + b"\xff", BB.PACK_ESHAPE
    elif what == "body3":
        body = good.index(b"\x84\x82\x82", b.txs[0][0] - 4)
        raw, want = good[:body] + b"\x83" + good[body + 1:], BB.PACK_ESHAPE
    elif what == "elem3":
        at = b.txs[0][0] - 1
        assert good[at] == 0x82
        raw, want = good[:at] + b"\x83" + good[at + 1:], BB.PACK_ESHAPE
    elif what == "tx_not_array":
        at = b.txs[1][0]
        raw, want = good[:at] + b"\xa0" + good[at + 1:], BB.PACK_ESHAPE
    elif what == "proof_size":
        at = good.index(b.claimed[2]) - 2
        assert good[at:at + 2] == b"\x58\x20"
        raw, want = good[:at] + b"\x58\x1f" + good[at + 3:], BB.PACK_ESIZE
    elif what == "trailing":
        raw, want = good + b"\x00", BB.PACK_ECBOR
    else:
        end = b.wits[1][0] + b.wits[1][1]
        assert good[end] == 0xFF
        raw, want = good[:end], BB.PACK_ECBOR
    assert BB.byron_block_status(raw) == want
