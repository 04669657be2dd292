#!/usr/bin/env python3
"""Extract the reference's golden BLOCK files into tests/golden/reference_blocks.json
(run in the build container only: /root/reference does not exist on the GPU box).

Data only -- the golden CBOR files the reference's serialisation tests hold,
as hex -- never reference source.  Sibling of tools/make_golden.py.
"""
import json
import os

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

SHELLEY = "ouroboros-consensus-shelley-test/test/golden"
CARDANO = "ouroboros-consensus-cardano-test/test/golden"
ERAS = ("Shelley", "Allegra", "Mary", "Byron_regular", "Byron_EBB")
FILES = ([("shelley_disk", f"{SHELLEY}/disk/Block"),
          ("shelley_n2n", f"{SHELLEY}/ShelleyNodeToNodeVersion1/Block")] +
         [(f"cardano_disk_{e}", f"{CARDANO}/disk/Block_{e}") for e in ERAS] +
         [(f"cardano_n2n_{e}", f"{CARDANO}/CardanoNodeToNodeVersion1/Block_{e}") for e in ERAS])


def main():
    blocks = []
    for name, rel in FILES:
        with open(os.path.join(REF, rel), "rb") as f:
            raw = f.read()
        blocks.append({"name": name, "source": rel, "byron": "Byron" in name, "raw": raw.hex()})
    # distinct contents only (a wire form can coincide with a disk form)
    seen, out = set(), []
    for b in blocks:
        if b["raw"] not in seen:
            seen.add(b["raw"])
            out.append(b)
    with open(os.path.join(OUT, "reference_blocks.json"), "w") as f:
        json.dump({"blocks": out}, f, indent=1, sort_keys=True)
    print(f"{len(out)} blocks, {sum(len(b['raw']) // 2 for b in out)} bytes")


if __name__ == "__main__":
    main()
