#!/usr/bin/env python3
"""Extract the reference fixtures that pin the header envelope into
tests/golden/reference_envelope.json (run where the reference tree is checked
out; pass its path).  DATA only: the two Byron headers cut from the golden
disk blocks, the golden Byron header hash, and the golden annotated tips.

  ouroboros-consensus-cardano-test/test/golden/disk/Block_Byron_regular
  .../Block_Byron_EBB, HeaderHash_Byron, AnnTip_{Byron,Shelley,Allegra,Mary}
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ouroboros_network_amd import header as H  # noqa: E402


def header_of_block(blk: bytes) -> bytes:
    """[kind, [header, body, extra]] -> the header item's bytes"""
    outer = H.array_items(blk, 0)
    inner = H.array_items(blk, outer[1][0])
    return blk[inner[0][0]:inner[0][1]]


def main(ref: str) -> None:
    d = os.path.join(ref, "ouroboros-consensus-cardano-test", "test", "golden", "disk")
    rd = lambda f: open(os.path.join(d, f), "rb").read()  # noqa: E731
    out = {
        "source": "ouroboros-consensus-cardano-test/test/golden/disk",
        "byron_regular_header": header_of_block(rd("Block_Byron_regular")).hex(),
        "byron_ebb_header": header_of_block(rd("Block_Byron_EBB")).hex(),
        "header_hash_byron": rd("HeaderHash_Byron").hex(),
    }
    for era in ("Byron", "Shelley", "Allegra", "Mary"):
        out["ann_tip_" + era.lower()] = rd("AnnTip_" + era).hex()
    with open(os.path.join(ROOT, "tests", "golden", "reference_envelope.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
