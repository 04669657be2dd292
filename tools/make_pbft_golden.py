#!/usr/bin/env python3
"""Extract the reference fixtures that pin the Byron ledger-view checks into
tests/golden/reference_pbft.json (run where the reference tree is checked out;
pass its path).  DATA only:

  ouroboros-consensus-byron-test/test/golden/
    ByronNodeToNodeVersion1/Header_regular
        the header's genesis key (the delegation certificate's issuer) and
        delegate key, each with KH(k) = Blake2b-224(SHA3-256(58 40 || k))
    disk/LedgerState
        the delegation map: the indefinite list of [genesis id, delegate id]
        pairs (28 bytes each) that holds the header's pair
    disk/ChainDepState
        the serialised signing window, [1, {genesis id: [slots]}]
    ByronNodeToNodeVersion1/GenTx
        the first 64-byte key of the transaction's witness, and its id
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ouroboros_network_amd import header as H  # noqa: E402
from ouroboros_network_amd import parse_byron_header  # noqa: E402


def kh(k: bytes) -> bytes:
    return hashlib.blake2b(hashlib.sha3_256(b"\x58\x40" + k).digest(), digest_size=28).digest()


def main(ref: str) -> None:
    g = os.path.join(ref, "ouroboros-consensus-byron-test", "test", "golden")
    rd = lambda f: open(os.path.join(g, f), "rb").read()  # noqa: E731
    raw = rd("ByronNodeToNodeVersion1/Header_regular")
    bh = parse_byron_header(raw)
    gid, did = kh(bh.issuer_xpub), kh(bh.delegate_xpub)
    ls = rd("disk/LedgerState")
    # the map's list: 9f, then array(2) of two bytes(28) per pair, then ff
    at = ls.index(b"\x9f\x82\x58\x1c" + gid + b"\x58\x1c" + did) + 1
    pairs = []
    while ls[at] != 0xFF:
        a, b = H.array_items(ls, at)
        pairs.append([H.bytes_at(ls, a[0]).hex(), H.bytes_at(ls, b[0]).hex()])
        at = b[1]
    tx = rd("ByronNodeToNodeVersion1/GenTx")
    kat = tx.index(b"\x58\x40") + 2
    tx_key = tx[kat:kat + 64]
    out = {
        "source": "ouroboros-consensus-byron-test/test/golden",
        "header": {
            "raw": raw.hex(),
            "genesis_vk": bh.issuer_xpub.hex(),
            "genesis_id": gid.hex(),
            "delegate_vk": bh.delegate_xpub.hex(),
            "delegate_id": did.hex(),
        },
        "delegation_map": pairs,   # [genesis id, delegate id]
        "chain_dep_state": rd("disk/ChainDepState").hex(),
        "gen_tx": {"key": tx_key.hex(), "id": kh(tx_key).hex()},
    }
    with open(os.path.join(ROOT, "tests", "golden", "reference_pbft.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
