#!/usr/bin/env python3
"""Extract the reference fixtures that pin the ledger-view checks' two hashes
into tests/golden/reference_ledger_view.json (run where the reference tree is
checked out; pass its path).  DATA only:

  ouroboros-consensus-shelley-test/test/golden/
    ShelleyNodeToClientVersion2/Result_StakeDistribution
        {pool id (28 B): [[stake num, stake den], hashVerKeyVRF (32 B)]}
    ShelleyNodeToClientVersion2/GenTx
        the example pool's id where it stands in the transaction: the staking
        credential of the first 57-byte address (header, payment, staking)
    disk/ChainDepState
        [1, [[1, 1], [[counters {pool id: n}, eta_v, eta_c], ...]]]: the OCERT
        counter map
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ouroboros_network_amd import header as H  # noqa: E402


def cbor_map(buf: bytes, i: int):
    """[(key span, value span)] of the definite-length map at i"""
    major, val, j = H._head(buf, i)
    assert major == 5
    out = []
    for _ in range(val):
        k = H.skip(buf, j)
        v = H.skip(buf, k)
        out.append(((j, k), (k, v)))
        j = v
    return out


def main(ref: str) -> None:
    g = os.path.join(ref, "ouroboros-consensus-shelley-test", "test", "golden")
    rd = lambda f: open(os.path.join(g, f), "rb").read()  # noqa: E731
    sd = rd("ShelleyNodeToClientVersion2/Result_StakeDistribution")
    (k, v), = cbor_map(sd, 0)
    stake, vrf = H.array_items(sd, v[0])
    num, den = H.array_items(sd, stake[0])
    tx = rd("ShelleyNodeToClientVersion2/GenTx")
    at = tx.index(b"\x58\x39")  # the first bytes(57): an address
    cds = rd("disk/ChainDepState")
    outer = H.array_items(cds, 0)
    inner = H.array_items(cds, outer[1][0])
    state = H.array_items(cds, inner[1][0])
    prtcl = H.array_items(cds, state[0][0])
    counters = {H.bytes_at(cds, ks[0]).hex(): H.uint_at(cds, vs[0])
                for ks, vs in cbor_map(cds, prtcl[0][0])}
    out = {
        "source": "ouroboros-consensus-shelley-test/test/golden",
        "stake_distribution": {
            "pool_id": H.bytes_at(sd, k[0]).hex(),
            "stake": [H.uint_at(sd, num[0]), H.uint_at(sd, den[0])],
            "vrf_hash": H.bytes_at(sd, vrf[0]).hex(),
        },
        "gen_tx_pool_id": tx[at + 2 + 29:at + 2 + 57].hex(),
        "chain_dep_state_counters": counters,
    }
    with open(os.path.join(ROOT, "tests", "golden", "reference_ledger_view.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
