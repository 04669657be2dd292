"""ouroboros-network_amd -- MI355X-native batch verifier for the Ouroboros
Praos/TPraos header-crypto hot path (Ed25519DSIGN, Sum6KES, PraosVRF draft-03)
and the Byron PBFT block signature (ByronDSIGN).

Importable as ``ouroboros_network_amd`` (repo-root symlink).  The compute path
is the gfx950 library ``lib/libouro_verify.so`` behind the C ABI in
``include/ouro_verify.h``; there is no CPU fallback.
"""
from . import _native
from ._native import DeviceError, NativeUnavailable
from .block import blake2b256_batch, parse_block, verify_block_integrity_cbor
from .byron_block import count_byron_blocks, parse_byron_block, verify_byron_block_integrity
from .byron_witness import (byron_witness_message, count_byron_block_witnesses,
                            parse_byron_witnesses, verify_byron_block_witnesses)
from .byron import (ByronDSIGN, dlg_cert_message, pack_byron_cbor, parse_byron_header,
                    verify_byron_cbor, verify_byron_headers, verify_delegation_certs)
from .dsign import Ed25519DSIGN
from .header import (chain_envelope_cbor, validate_chain_cbor, validate_chain_ledger_cbor,
                     verify_chain_cbor, verify_headers_cbor, verify_integrity_cbor)
from .ledger import (Counters, GenesisDelegs, Globals, LedgerViews, counter_fold,
                     ledger_checks)
from .kes import Sum6KES, kes_period
from .pbft import (PBftState, PBftViews, byron_key_hash, pbft_checks, pbft_rule,
                   pbft_window_fold, validate_chain_pbft_cbor)
from .leader import ActiveSlotCoeff, leader_schedule, leader_vrfs
from .tpraos import EpochNonces, HeaderBatch, first_invalid, verify_headers, verify_headers_multi
from .vrf import PraosVRF
from .witness import count_block_witnesses, parse_witnesses, verify_block_witnesses

__all__ = [
    "ActiveSlotCoeff",
    "ByronDSIGN",
    "Counters",
    "DeviceError",
    "Ed25519DSIGN",
    "EpochNonces",
    "Globals",
    "GenesisDelegs",
    "HeaderBatch",
    "LedgerViews",
    "NativeUnavailable",
    "PBftState",
    "PBftViews",
    "PraosVRF",
    "Sum6KES",
    "blake2b256_batch",
    "byron_key_hash",
    "byron_witness_message",
    "chain_envelope_cbor",
    "count_block_witnesses",
    "count_byron_block_witnesses",
    "count_byron_blocks",
    "counter_fold",
    "first_invalid",
    "kes_period",
    "leader_schedule",
    "leader_vrfs",
    "ledger_checks",
    "dlg_cert_message",
    "pack_byron_cbor",
    "parse_block",
    "parse_byron_block",
    "parse_byron_header",
    "parse_byron_witnesses",
    "parse_witnesses",
    "pbft_checks",
    "pbft_rule",
    "pbft_window_fold",
    "validate_chain_cbor",
    "validate_chain_ledger_cbor",
    "validate_chain_pbft_cbor",
    "verify_block_integrity_cbor",
    "verify_block_witnesses",
    "verify_byron_block_integrity",
    "verify_byron_block_witnesses",
    "verify_byron_cbor",
    "verify_byron_headers",
    "verify_chain_cbor",
    "verify_delegation_certs",
    "verify_headers",
    "verify_headers_cbor",
    "verify_headers_multi",
    "verify_integrity_cbor",
]


def library_path() -> str:
    return _native.LIB_PATH
