"""ctypes mirror of include/ibftgpu.h — the batch form of go-ibft's Verifier.

Method names follow the reference interface they replace
(/root/reference/core/backend.go:37-56):

    IsValidProposalHash(proposal, hash)        -> BatchVerifier.is_valid_proposal_hash(raw, round, hashes)
    IsValidCommittedSeal(proposalHash, seal)   -> BatchVerifier.is_valid_committed_seal(hashes, seals, signers)
    IsValidValidator(msg)                      -> BatchVerifier.is_valid_validator(payloads, sigs, froms)
    ValidatorManager.HasQuorum(senders)        -> the Tally returned next to each verdict array

Every method returns a numpy bool array (one verdict per row) — the value the
per-message reference predicate would have returned.  No CPU fallback: a missing
library or device raises ``GpuUnavailable``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .build import LIB

FLAG_STRICT_LOW_S = 1
FLAG_PUBKEY_CACHE = 2   # warm path: verify against per-validator tables once a key has been recovered
FLAG_CERT_DEDUP = 4     # certificate calls judge each distinct (digest, signature, From) once (IBFT_CERT_DEDUP=0|1 overrides)
FLAG_WIRE_RECODE = 8    # the flat wire calls also judge non-canonical PREPARE / COMMIT encodings (IBFT_WIRE_RECODE=0|1 overrides)
ROW_NIL, ROW_BADLEN, ROW_HASH_BAD = 1, 2, 4
KERNEL_AUTO, KERNEL_LANE, KERNEL_WAVE = 0, 1, 2
SIGN_NONCE_KECCAK, SIGN_NONCE_RFC6979 = 0, 1   # IBFT_SIGN_NONCE_*
SIGN_NONCES = {"keccak": SIGN_NONCE_KECCAK, "rfc6979": SIGN_NONCE_RFC6979}

EXPORTS = [
    "ibft_version", "ibft_strerror", "ibft_last_error", "ibft_ctx_create", "ibft_ctx_destroy",
    "ibft_set_validators", "ibft_verify_hashes", "ibft_proposal_hash", "ibft_verify_seals",
    "ibft_verify_senders", "ibft_tally", "ibft_seals_stage", "ibft_seals_launch", "ibft_seals_fetch",
    "ibft_seals_device_ptrs", "ibft_seals_export", "ibft_last_kernel_ms", "ibft_cache_stats", "ibft_last_dispatch", "ibft_sync",
    "ibft_verify_senders_wire", "ibft_wire_stage_seals", "ibft_seals_export_on",
    "ibft_set_validators_u256", "ibft_last_tally_wide",
    "ibft_shard_range", "ibft_exchange_layout", "ibft_comm_unique_id", "ibft_comm_init", "ibft_comm_destroy",
    "ibft_seals_exchange", "ibft_seals_fetch_merged", "ibft_seals_run", "ibft_verify_hashes_digest", "ibft_set_kernel_timing",
    "ibft_group_create", "ibft_group_destroy", "ibft_group_size", "ibft_group_ctx", "ibft_group_set_validators",
    "ibft_group_set_validators_u256", "ibft_group_verify_seals", "ibft_group_verify_senders", "ibft_group_verify_messages", "ibft_group_verify_certificates_wire",
    "ibft_group_is_local", "ibft_sign_seals", "ibft_verify_messages", "ibft_pinned_alloc", "ibft_pinned_free", "ibft_column_stats",
    "ibft_verify_messages_wire", "ibft_forget_proposal", "ibft_verify_certificates_wire", "ibft_keccak256",
    "ibft_cache_memory", "ibft_tally_prepare", "ibft_comm_info", "ibft_set_seal_digest", "ibft_group_set_seal_digest",
    "ibft_seals_stage_next", "ibft_seals_swap", "ibft_last_cold_table", "ibft_seals_submit", "ibft_seals_collect",
    "ibft_comm_preload", "ibft_issue_probe", "ibft_seals_rows", "ibft_pipeline_stats", "ibft_verify_block_seals",
    "ibft_block_seals_submit", "ibft_block_seals_collect", "ibft_block_seals_pending",
    "ibft_block_seals_submit_raw", "ibft_recover_block_seals_submit", "ibft_recover_block_seals_submit_raw",
    "ibft_block_seals_collect_ex", "ibft_block_seals_pending_ex",
    "ibft_recover_seals", "ibft_recover_block_seals",
    "ibft_proposal_hashes", "ibft_verify_block_seals_raw", "ibft_recover_block_seals_raw",
    "ibft_set_validator_sets", "ibft_set_validator_sets_u256", "ibft_validator_sets_info",
    "ibft_verify_block_seals_sets", "ibft_recover_block_seals_sets",
    "ibft_verify_block_seals_sets_raw", "ibft_recover_block_seals_sets_raw", "ibft_block_seals_submit_sets",
    "ibft_block_seals_submit_sets_raw", "ibft_recover_block_seals_submit_sets", "ibft_recover_block_seals_submit_sets_raw",
    "ibft_sign_seals_ex", "ibft_sign_messages_wire", "ibft_sign_envelopes_wire", "ibft_judge_certificates_wire",
    "ibft_cert_stats", "ibft_pipeline_stats_ex", "ibft_cache_form", "ibft_wire_stats",
    "ibft_set_proposers", "ibft_proposers_info", "ibft_decide_certificates_wire", "ibft_decide_round_changes_wire",
    "ibft_set_height_sets", "ibft_height_sets_info", "ibft_verify_senders_wire_sets", "ibft_verify_senders_wire_views",
    "ibft_verify_messages_wire_views", "ibft_wire_seal_stats",
]
# exports younger than version 3: the version that brought them (ibft_verify_block_seals, the streamed ibft_block_seals_* and
# ibft_recover_seals / ibft_recover_block_seals, ibft_proposal_hashes / the two _raw block calls and the validator-set family
# (ibft_set_validator_sets …, the two _sets block calls, their two _raw and four streamed forms), ibft_sign_seals_ex, ibft_sign_messages_wire and ibft_judge_certificates_wire came without a version step: an
# older build simply lacks them, and the BatchVerifier methods raise GpuUnavailable there)
EXPORTS_SINCE = {"ibft_pipeline_stats": 4}
OPTIONAL_EXPORTS = {"ibft_verify_block_seals", "ibft_block_seals_submit", "ibft_block_seals_collect", "ibft_block_seals_pending",
                    "ibft_block_seals_submit_raw", "ibft_recover_block_seals_submit", "ibft_recover_block_seals_submit_raw",
                    "ibft_block_seals_collect_ex", "ibft_block_seals_pending_ex",
                    "ibft_recover_seals", "ibft_recover_block_seals",
                    "ibft_proposal_hashes", "ibft_verify_block_seals_raw", "ibft_recover_block_seals_raw",
                    "ibft_set_validator_sets", "ibft_set_validator_sets_u256", "ibft_validator_sets_info",
                    "ibft_verify_block_seals_sets", "ibft_recover_block_seals_sets",
                    "ibft_verify_block_seals_sets_raw", "ibft_recover_block_seals_sets_raw", "ibft_block_seals_submit_sets",
                    "ibft_block_seals_submit_sets_raw", "ibft_recover_block_seals_submit_sets", "ibft_recover_block_seals_submit_sets_raw",
                    "ibft_sign_seals_ex", "ibft_sign_messages_wire", "ibft_sign_envelopes_wire", "ibft_judge_certificates_wire",
                    "ibft_cert_stats", "ibft_pipeline_stats_ex", "ibft_cache_form", "ibft_wire_stats",
                    "ibft_set_proposers", "ibft_proposers_info", "ibft_decide_certificates_wire", "ibft_decide_round_changes_wire",
                    "ibft_set_height_sets", "ibft_height_sets_info", "ibft_verify_senders_wire_sets", "ibft_verify_senders_wire_views",
                    "ibft_verify_messages_wire_views", "ibft_wire_seal_stats"}
SIGN_MESSAGE_MAX = 218   # IBFT_SIGN_MESSAGE_MAX: the longest message ibft_sign_messages_wire emits
ENVELOPE_HEAD_MAX = 121  # the most ibft_sign_envelopes_wire puts in front of a body (sign_envelope_dev.h)
MSG_PREPARE, MSG_COMMIT = 1, 2
COMM_ID_BYTES = 128
E_RCCL = -8

WIRE_OK, WIRE_NEEDS_HOST = 0, 1
WIRE_CLASS_NEEDS_HOST, WIRE_CLASS_CLOSURE = 1, 2
# ibft_wire_row_t (include/ibftgpu.h)
WIRE_ROW = np.dtype([("height", "<u8"), ("round", "<u8"), ("status", "u1"), ("type", "u1"), ("payload_kind", "u1"),
                     ("has_view", "u1"), ("hash_len", "u1"), ("seal_len", "u1"), ("from_len", "u1"), ("sig_len", "u1"),
                     ("from", "u1", 20), ("proposal_hash", "u1", 32), ("pad", "u1", 4)])
assert WIRE_ROW.itemsize == 80
# ibft_cert_node_t (include/ibftgpu.h)
CERT_NODE = np.dtype([("off", "<u4"), ("len", "<u4"), ("parent", "<u4"), ("ordinal", "<u4"), ("first_child", "<u4"),
                      ("n_children", "<u4"), ("raw_off", "<u4"), ("raw_len", "<u4"), ("proposal_round", "<u8"),
                      ("cut0", "<u4"), ("cut1", "<u4"), ("level", "u1"), ("role", "u1"), ("flags", "u1"), ("pad", "u1", 5)])
assert CERT_NODE.itemsize == 56
CERT_CLASS_NEEDS_HOST, CERT_CLASS_DIGEST_BY_HOST, CERT_CLASS_PROPOSAL_BY_HOST = 1, 2, 4
CERT_NO_PARENT = 0xFFFFFFFF
# ibft_cert_verdict_t (include/ibftgpu.h): one record per carrier of ibft_judge_certificates_wire
CERT_VERDICT = np.dtype([("row", "<u4"), ("first_child", "<u4"), ("n_children", "<u4"), ("first_child_cert", "<u4"), ("rcc_rows", "<u4"),
                         ("pc", "i1"), ("rcc", "i1"), ("cls", "u1"), ("bits", "u1"), ("type", "u1"), ("role", "u1"), ("level", "u1"),
                         ("from_len", "u1"), ("reserved", "<u4"), ("height", "<u8"), ("round", "<u8"), ("pc_round", "<u8"),
                         ("from", "u1", 20), ("pc_from", "u1", 20), ("pc_hash", "u1", 32)])
assert CERT_VERDICT.itemsize == 128
CERT_NO_RECORD = 0xFFFFFFFF
CERT_BIT_SENDER, CERT_BIT_HASH, CERT_BIT_SELF, CERT_BIT_HAS_PROPOSAL, CERT_BIT_HAS_CERTIFICATE = 1, 2, 4, 8, 16
# ibft_cert_decision_t (include/ibftgpu.h): one decision per record of ibft_decide_certificates_wire
CERT_DECISION = np.dtype([("valid_pc", "i1"), ("round_change", "i1"), ("proposal", "i1"), ("flags", "u1"), ("prepared_record", "<u4"),
                          ("prepared_round", "<u8"), ("prepared_hash", "u1", 32), ("reserved", "u1", 16)])
assert CERT_DECISION.itemsize == 64
CERT_DECISION_HAS_PREPARED = 1
PROPOSER_ROUNDS_MAX = 4096   # IBFT_PROPOSER_ROUNDS_MAX
# ibft_wire_view_t (include/ibftgpu.h); tally: ibft_tally_t, field for field the Tally structure
WIRE_VIEW = np.dtype([("height", "<u8"), ("round", "<u8"), ("set", "<i4"), ("first_row", "<u4"), ("rows", "<u4"), ("stored_rows", "<u4"),
                      ("type", "u1"), ("hash_len", "u1"), ("prepare_rule", "u1"), ("pad", "u1", 5), ("proposal_hash", "u1", 32),
                      ("tally", [("quorum_lo", "<u8"), ("quorum_hi", "<u8"), ("power_lo", "<u8"), ("power_hi", "<u8"),
                                 ("valid_rows", "<u4"), ("distinct_senders", "<u4"), ("has_quorum", "<u4"), ("shard_overlap", "<u4"),
                                 ("proposer_rows", "<u4"), ("reserved", "<u4")])])
assert WIRE_VIEW.itemsize == 128
# ibft_rc_query_t / ibft_rc_record_t / ibft_rc_answer_t (include/ibftgpu.h): ibft_decide_round_changes_wire
RC_QUERY = np.dtype([("height", "<u8"), ("round", "<u8"), ("min_round", "<u8"), ("has_accepted_proposal", "<u4"), ("reserved", "<u4")])
RC_RECORD = np.dtype([("height", "<u8"), ("round", "<u8"), ("first_row", "<u4"), ("rows", "<u4"), ("stored_rows", "<u4"), ("yes_rows", "<u4"),
                      ("open_rows", "<u4"), ("has_quorum", "i1"), ("pad", "u1", 3), ("open_power_lo", "<u8"), ("open_power_hi", "<u8"),
                      ("tally", WIRE_VIEW.fields["tally"][0]), ("reserved", "u1", 16)])
RC_ANSWER = np.dtype([("extended", "i1"), ("pad", "u1", 3), ("flags", "<u4"), ("record", "<u4"), ("most_record", "<u4"), ("round", "<u8"),
                      ("most_round", "<u8"), ("most_rows", "<u4"), ("records_of_height", "<u4"), ("unjudged_rows", "<u4"), ("reserved", "u1", 20)])
assert (RC_QUERY.itemsize, RC_RECORD.itemsize, RC_ANSWER.itemsize) == (32, 128, 64)
RC_VIEW_NONE, RC_VIEW_OVER, RC_OVER = -1, -2, 1   # IBFT_RC_VIEW_NONE, IBFT_RC_VIEW_OVER, IBFT_RC_OVER
WIRE_VIEW_SEAL_RULE = 0      # IBFT_WIRE_VIEW_SEAL_RULE: pad[0] = 1 — the record's tally counts only rows whose committed seal verifies


class GpuUnavailable(RuntimeError):
    pass


class Cfg(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32), ("max_rows", C.c_uint32),
                ("kernel", C.c_uint32)]


class Tally(C.Structure):
    _fields_ = [("quorum_lo", C.c_uint64), ("quorum_hi", C.c_uint64),
                ("power_lo", C.c_uint64), ("power_hi", C.c_uint64),
                ("valid_rows", C.c_uint32), ("distinct_senders", C.c_uint32),
                ("has_quorum", C.c_uint32), ("shard_overlap", C.c_uint32),
                ("proposer_rows", C.c_uint32), ("reserved", C.c_uint32)]

    @property
    def power(self) -> int:
        return self.power_lo | (self.power_hi << 64)

    @property
    def quorum(self) -> int:
        return self.quorum_lo | (self.quorum_hi << 64)


class TallyWide(C.Structure):
    """ibft_tally_wide_t: full-width (320-bit) power and quorum of the last tally."""
    _fields_ = [("quorum_w", C.c_uint64 * 5), ("power_w", C.c_uint64 * 5), ("has_quorum", C.c_uint32),
                ("reserved", C.c_uint32)]

    @property
    def power(self) -> int:
        return sum(int(w) << (64 * i) for i, w in enumerate(self.power_w))

    @property
    def quorum(self) -> int:
        return sum(int(w) << (64 * i) for i, w in enumerate(self.quorum_w))


def powers_be32(powers) -> np.ndarray:
    """list of Python ints → n × 32 big-endian bytes (what big.Int.FillBytes(make([]byte, 32)) produces)"""
    return np.frombuffer(b"".join(int(p).to_bytes(32, "big") for p in powers), dtype=np.uint8).reshape(-1, 32).copy()


def _block_call_argtypes() -> dict:
    """export → argtypes of the sixteen block calls (include/ibftgpu.h), from what each is given: the head (hashes: one pointer,
    proposals: three), seal_off, a block_set column (the _sets calls), n_blocks, sig65, signer20 unless the seals are bare,
    pre_flags; the synchronous calls go on with their out buffers: the block hashes (_raw), signers and indices (recover),
    verdict words, tallies"""
    vp, out = C.c_void_p, {}
    for raw in (False, True):
        for sets in (False, True):
            for bare in (False, True):
                given = [vp] * (5 if raw else 3) + [vp] * sets + [C.c_size_t, vp] + [vp] * (not bare) + [vp]   # (the context first)
                suffix = ("_sets" if sets else "") + ("_raw" if raw else "")
                out["ibft_" + ("recover" if bare else "verify") + "_block_seals" + suffix] = given + [vp] * (raw + 2 * bare + 2)
                out["ibft_" + ("recover_" if bare else "") + "block_seals_submit" + suffix] = given
    return out


_lib = None
ABI_VERSION = 4   # include/ibftgpu.h: ibft_version()  (3: the round-5/6 exports; 4: ibft_pipeline_stats)


def load_library() -> C.CDLL:
    """dlopen libibftgpu.so and declare the prototypes (works without a GPU)."""
    global _lib
    if _lib is not None:
        return _lib
    lib_path = os.environ.get("IBFT_GPU_LIB") or LIB   # IBFT_GPU_LIB: A/B experiments with another build of the library
    if not os.path.exists(lib_path):
        raise GpuUnavailable(f"{lib_path} is not built — run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(lib_path)
    vp = C.c_void_p
    L.ibft_version.restype = C.c_int
    # IBFT_MIN_ABI (A/B tools only: tools/kernel_ab.py against an OLDER build of the library): accept a library of that version and
    # do without the exports that came after it — never below 3 (the struct layouts changed there)
    need = max(3, min(ABI_VERSION, int(os.environ.get("IBFT_MIN_ABI", ABI_VERSION))))
    if L.ibft_version() < need:   # a stale .so writes past the caller's ibft_tally_t (48 → 56 bytes at version 2)
        raise GpuUnavailable(f"{lib_path}: ibft_version() = {L.ibft_version()}, this binding needs >= {need} — rebuild")
    later = {name for name, since in EXPORTS_SINCE.items() if since > need}
    later |= {name for name in OPTIONAL_EXPORTS if not hasattr(L, name)}
    missing = [name for name in EXPORTS if name not in later and not hasattr(L, name)]   # BEFORE the prototypes below touch any of them
    if missing:
        raise GpuUnavailable(f"{lib_path} lacks {', '.join(missing)} — a stale build: rebuild")
    L.ibft_strerror.argtypes = [C.c_int]; L.ibft_strerror.restype = C.c_char_p
    L.ibft_last_error.argtypes = [vp]; L.ibft_last_error.restype = C.c_char_p
    L.ibft_ctx_create.argtypes = [C.POINTER(Cfg), C.POINTER(vp)]
    L.ibft_ctx_destroy.argtypes = [vp]; L.ibft_ctx_destroy.restype = None
    L.ibft_set_validators.argtypes = [vp, C.c_uint64, vp, vp, C.c_size_t]
    L.ibft_verify_hashes.argtypes = [vp, vp, C.c_size_t, C.c_uint64, vp, vp, C.c_size_t, vp]
    L.ibft_proposal_hash.argtypes = [vp, vp, C.c_size_t, C.c_uint64, vp]
    L.ibft_verify_hashes_digest.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
    L.ibft_verify_seals.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, vp, C.POINTER(Tally)]
    L.ibft_verify_senders.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, vp, C.POINTER(Tally)]
    L.ibft_tally.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(Tally)]
    L.ibft_tally_prepare.argtypes = [vp, vp, vp, C.c_size_t, vp, C.POINTER(Tally)]
    L.ibft_set_seal_digest.argtypes = [vp, C.c_uint32, vp, C.c_size_t]
    L.ibft_group_set_seal_digest.argtypes = [vp, C.c_uint32, vp, C.c_size_t]
    L.ibft_comm_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    L.ibft_seals_stage.argtypes = [vp, vp, vp, vp, vp, C.c_size_t]
    L.ibft_seals_launch.argtypes = [vp, C.c_uint32]
    L.ibft_seals_fetch.argtypes = [vp, vp, C.POINTER(Tally)]
    L.ibft_seals_run.argtypes = [vp, vp, C.POINTER(Tally)]
    L.ibft_seals_stage_next.argtypes = [vp, vp, vp, vp, vp, C.c_size_t]
    L.ibft_seals_swap.argtypes = [vp, C.c_int]
    L.ibft_last_cold_table.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.ibft_seals_submit.argtypes = [vp]
    L.ibft_seals_collect.argtypes = [vp, vp, C.POINTER(Tally)]
    L.ibft_sign_seals.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp]
    L.ibft_verify_messages_wire.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint64, C.c_uint64, vp, C.c_size_t, C.c_uint64, vp, vp, vp, vp, vp,
                                            vp, C.POINTER(Tally)]
    L.ibft_forget_proposal.argtypes = [vp]
    L.ibft_pinned_alloc.argtypes = [C.c_size_t]; L.ibft_pinned_alloc.restype = vp
    L.ibft_pinned_free.argtypes = [vp]; L.ibft_pinned_free.restype = None
    L.ibft_column_stats.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.ibft_verify_messages.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_uint64, vp, vp, vp, vp,
                                       C.POINTER(Tally)]
    L.ibft_seals_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp)]
    L.ibft_seals_export.argtypes = [vp, vp, vp]
    L.ibft_seals_export_on.argtypes = [vp, vp, vp, vp]
    L.ibft_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    L.ibft_set_kernel_timing.argtypes = [vp, C.c_uint32]
    L.ibft_cache_stats.argtypes = [vp] + [C.POINTER(C.c_uint32)] * 4
    L.ibft_last_dispatch.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.ibft_sync.argtypes = [vp]
    L.ibft_issue_probe.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.ibft_seals_rows.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    optional = _block_call_argtypes()
    optional.update({   # the other exports an older build may lack
        "ibft_pipeline_stats": [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
        "ibft_pipeline_stats_ex": [vp] + [C.POINTER(C.c_uint32)] * 3,
        "ibft_sign_seals_ex": [vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp, vp],
        "ibft_sign_messages_wire": [vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_uint32, vp, C.c_size_t, vp, vp, vp],
        "ibft_sign_envelopes_wire": [vp, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.c_uint32, vp, C.c_size_t, vp, vp, vp],
        "ibft_recover_seals": [vp, vp, vp, vp, C.c_size_t, vp, vp, vp, C.POINTER(Tally)],
        "ibft_proposal_hashes": [vp, vp, vp, vp, C.c_size_t, vp],
        "ibft_set_validator_sets": [vp, C.c_size_t, vp, vp, vp, vp],
        "ibft_set_validator_sets_u256": [vp, C.c_size_t, vp, vp, vp, vp],
        "ibft_validator_sets_info": [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)],
        "ibft_set_height_sets": [vp, C.c_size_t, vp, vp],
        "ibft_height_sets_info": [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
        "ibft_verify_senders_wire_sets": [vp, vp, vp, C.c_size_t, vp, vp, vp, vp, vp],
        "ibft_verify_senders_wire_views": [vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_uint32)],
        "ibft_verify_messages_wire_views": [vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_uint32), vp],
        "ibft_wire_seal_stats": [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
        "ibft_block_seals_collect": [vp, vp, vp],
        "ibft_block_seals_pending": [vp] + [C.POINTER(C.c_uint32)] * 3,
        "ibft_block_seals_collect_ex": [vp, vp, vp, vp, vp, vp],
        "ibft_block_seals_pending_ex": [vp] + [C.POINTER(C.c_uint32)] * 4,
    })
    for name, argtypes in optional.items():
        if hasattr(L, name):
            getattr(L, name).argtypes = argtypes
    L.ibft_verify_senders_wire.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, C.POINTER(Tally)]
    L.ibft_wire_stage_seals.argtypes = [vp]
    L.ibft_verify_certificates_wire.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), vp, vp, vp, vp, vp, vp]
    if hasattr(L, "ibft_judge_certificates_wire"):
        L.ibft_judge_certificates_wire.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                                   vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "ibft_decide_certificates_wire"):
        L.ibft_decide_certificates_wire.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                                    vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "ibft_decide_round_changes_wire"):
        L.ibft_decide_round_changes_wire.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                                     vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
    if hasattr(L, "ibft_set_proposers"):
        L.ibft_set_proposers.argtypes = [vp, C.c_uint64, C.c_uint64, vp, C.c_size_t]
    if hasattr(L, "ibft_proposers_info"):
        L.ibft_proposers_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    if hasattr(L, "ibft_cert_stats"):
        L.ibft_cert_stats.argtypes = [vp] + [C.POINTER(C.c_uint32)] * 4
    if hasattr(L, "ibft_wire_stats"):
        L.ibft_wire_stats.argtypes = [vp] + [C.POINTER(C.c_uint32)] * 3
    L.ibft_set_validators_u256.argtypes = [vp, C.c_uint64, vp, vp, C.c_size_t]
    L.ibft_last_tally_wide.argtypes = [vp, C.POINTER(TallyWide)]
    L.ibft_shard_range.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ibft_exchange_layout.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.ibft_comm_unique_id.argtypes = [vp]
    L.ibft_comm_init.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.ibft_comm_destroy.argtypes = [vp]
    L.ibft_seals_exchange.argtypes = [vp, C.c_uint64]
    L.ibft_seals_fetch_merged.argtypes = [vp, vp, C.POINTER(Tally)]
    L.ibft_group_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.ibft_group_destroy.argtypes = [vp]; L.ibft_group_destroy.restype = None
    L.ibft_group_size.argtypes = [vp]; L.ibft_group_size.restype = C.c_uint32
    L.ibft_group_ctx.argtypes = [vp, C.c_uint32]; L.ibft_group_ctx.restype = vp
    L.ibft_group_set_validators.argtypes = [vp, C.c_uint64, vp, vp, C.c_size_t]
    L.ibft_group_set_validators_u256.argtypes = [vp, C.c_uint64, vp, vp, C.c_size_t]
    L.ibft_group_verify_seals.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, vp, C.POINTER(Tally)]
    L.ibft_group_verify_senders.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, vp, C.POINTER(Tally)]
    L.ibft_group_verify_messages.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_uint64, vp,
                                             vp, vp, vp, C.POINTER(Tally)]
    L.ibft_group_verify_certificates_wire.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
    L.ibft_group_is_local.argtypes = [vp]
    L.ibft_keccak256.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp]
    L.ibft_cache_memory.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    if hasattr(L, "ibft_cache_form"):
        L.ibft_cache_form.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    for name in EXPORTS:  # fail loudly on a stale build that lacks a declared symbol
        if name not in later:
            getattr(L, name)
    _lib = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _judge_certificates_wire(L, handle, chk, wire, off, rows_cap: int, certs_cap: int | None, per_row: bool, decide: bool = False):
    """ibft_judge_certificates_wire on one context → (certs[CERT_VERDICT], n_rows, per-row outputs or None); the per-row outputs
    are verify_certificates_wire's tuple without its first element.  decide: ibft_decide_certificates_wire →
    (certs, decisions[CERT_DECISION], n_rows, per-row outputs or None)"""
    name = "ibft_decide_certificates_wire" if decide else "ibft_judge_certificates_wire"
    if not hasattr(L, name):
        raise GpuUnavailable(f"this build of libibftgpu.so has no {name} — rebuild")
    wb = _bytes_col(wire)
    off = np.ascontiguousarray(off, dtype=np.uint32)
    n = len(off) - 1
    cap = int(rows_cap)
    ccap = cap if certs_cap is None else int(certs_cap)
    certs = np.zeros(max(ccap, 1), dtype=CERT_VERDICT)
    nodes = rows = cls = ms = mh = mself = None
    if per_row:
        words = (cap + 63) // 64 or 1
        nodes = np.zeros(max(cap, 1), dtype=CERT_NODE)
        rows = np.zeros(max(cap, 1), dtype=WIRE_ROW)
        cls = np.zeros(max(cap, 1), dtype=np.uint8)
        ms, mh, mself = (np.zeros(words, dtype=np.uint64) for _ in range(3))
    n_rows, n_certs = C.c_size_t(0), C.c_size_t(0)
    decisions = np.zeros(max(ccap, 1), dtype=CERT_DECISION) if decide else None
    if decide:
        chk(L.ibft_decide_certificates_wire(handle, _p(wb), _p(off), n, cap, ccap, C.byref(n_rows), C.byref(n_certs), _p(certs), _p(decisions),
                                            _p(nodes), _p(rows), _p(cls), _p(ms), _p(mh), _p(mself)), name)
    else:
        chk(L.ibft_judge_certificates_wire(handle, _p(wb), _p(off), n, cap, ccap, C.byref(n_rows), C.byref(n_certs), _p(certs), _p(nodes),
                                           _p(rows), _p(cls), _p(ms), _p(mh), _p(mself)), name)
    k = int(n_rows.value)
    out = None
    if per_row:
        out = (nodes[:k], rows[:k], cls[:k], mask_to_bool(ms, k), mask_to_bool(mh, k), mask_to_bool(mself, k))
    if decide:
        return certs[:int(n_certs.value)], decisions[:int(n_certs.value)], k, out
    return certs[:int(n_certs.value)], k, out


def rc_query(height: int, round_: int, has_accepted_proposal: bool = False, min_round: int = 0) -> np.ndarray:
    """an ibft_rc_query_t: the node's view, whether it has accepted a proposal, GetMostRoundChangeMessages' min_round"""
    q = np.zeros(1, dtype=RC_QUERY)
    q["height"], q["round"], q["min_round"], q["has_accepted_proposal"] = int(height), int(round_), int(min_round), 1 if has_accepted_proposal else 0
    return q


def _decide_round_changes_wire(L, handle, chk, wire, off, query, rows_cap: int, certs_cap: int | None, rc_cap: int | None, per_row: bool):
    """ibft_decide_round_changes_wire on one context → (certs, decisions, n_rows, per-row outputs or None, rc) with rc =
    (rc_view[n], rc_stored[n] as bools, records[min(n_rc, rc_cap)] as RC_RECORD, n_rc, answer as an RC_ANSWER scalar or None)"""
    name = "ibft_decide_round_changes_wire"
    if not hasattr(L, name):
        raise GpuUnavailable(f"this build of libibftgpu.so has no {name} — rebuild")
    wb = _bytes_col(wire)
    off = np.ascontiguousarray(off, dtype=np.uint32)
    n = len(off) - 1
    cap = int(rows_cap)
    ccap = cap if certs_cap is None else int(certs_cap)
    rcap = n if rc_cap is None else int(rc_cap)
    certs = np.zeros(max(ccap, 1), dtype=CERT_VERDICT)
    decisions = np.zeros(max(ccap, 1), dtype=CERT_DECISION)
    nodes = rows = cls = ms = mh = mself = None
    if per_row:
        words = (cap + 63) // 64 or 1
        nodes = np.zeros(max(cap, 1), dtype=CERT_NODE)
        rows = np.zeros(max(cap, 1), dtype=WIRE_ROW)
        cls = np.zeros(max(cap, 1), dtype=np.uint8)
        ms, mh, mself = (np.zeros(words, dtype=np.uint64) for _ in range(3))
    q = None if query is None else np.ascontiguousarray(query, dtype=RC_QUERY).reshape(1)
    rc_view = np.zeros(max(n, 1), dtype=np.int32)
    rc_stored = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
    recs = np.zeros(max(min(rcap, n), 1), dtype=RC_RECORD)
    answer = np.zeros(1, dtype=RC_ANSWER)
    n_rows, n_certs, n_rc = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    chk(L.ibft_decide_round_changes_wire(handle, _p(wb), _p(off), n, cap, ccap, C.byref(n_rows), C.byref(n_certs), _p(certs), _p(decisions),
                                         _p(nodes), _p(rows), _p(cls), _p(ms), _p(mh), _p(mself), _p(q), _p(rc_view), _p(rc_stored), _p(recs),
                                         rcap, C.byref(n_rc), _p(answer)), name)
    k = int(n_rows.value)
    out = None
    if per_row:
        out = (nodes[:k], rows[:k], cls[:k], mask_to_bool(ms, k), mask_to_bool(mh, k), mask_to_bool(mself, k))
    filled = min(int(n_rc.value), rcap, n)
    rc = (rc_view[:n], mask_to_bool(rc_stored, n), recs[:filled], int(n_rc.value), None if q is None else answer[0])
    return certs[:int(n_certs.value)], decisions[:int(n_certs.value)], k, out, rc


def _set_proposers(L, handle, chk, height: int, first_round: int, addrs) -> None:
    """ibft_set_proposers on one context: addrs[k] (20 bytes) proposes round first_round + k of `height`; no addrs: the table is cleared"""
    if not hasattr(L, "ibft_set_proposers"):
        raise GpuUnavailable("this build of libibftgpu.so has no ibft_set_proposers — rebuild")
    flat = addrs if isinstance(addrs, np.ndarray) else np.frombuffer(b"".join(bytes(x) for x in addrs), dtype=np.uint8)
    a = np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1, 20)   # raises for anything that is not 20 bytes per round
    chk(L.ibft_set_proposers(handle, int(height), int(first_round), _p(a) if len(a) else None, len(a)), "ibft_set_proposers")


def _proposers_info(L, handle, chk):
    """ibft_proposers_info on one context → (height, first_round, n_rounds); n_rounds == 0: no table"""
    if not hasattr(L, "ibft_proposers_info"):
        raise GpuUnavailable("this build of libibftgpu.so has no ibft_proposers_info — rebuild")
    h, f, n = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    chk(L.ibft_proposers_info(handle, C.byref(h), C.byref(f), C.byref(n)), "ibft_proposers_info")
    return int(h.value), int(f.value), int(n.value)


class _PinnedOwner:
    """keeps one ibft_pinned_alloc block alive for as long as a numpy view of it exists"""

    def __init__(self, nbytes: int):
        self._L = load_library()
        self.ptr = self._L.ibft_pinned_alloc(nbytes)
        if not self.ptr:
            raise GpuUnavailable("ibft_pinned_alloc failed")
        self.buf = (C.c_uint8 * max(nbytes, 1)).from_address(self.ptr)

    def __del__(self):
        if getattr(self, "ptr", None):
            self._L.ibft_pinned_free(self.ptr)
            self.ptr = None


def pinned_copy(a) -> np.ndarray:
    """a copy of `a` (array or bytes) in page-locked memory from ibft_pinned_alloc: what a caller's flatten step
    should write its columns into (include/ibftgpu.h, "pinned column buffers")"""
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    a = np.ascontiguousarray(a)
    own = _PinnedOwner(a.nbytes)
    out = np.frombuffer(own.buf, dtype=a.dtype, count=a.size).reshape(a.shape)  # .base chain keeps `own.buf` alive
    out[...] = a
    own.buf._owner = own  # the view's base chain reaches the ctypes array, which now keeps the block's owner alive
    return out


def _bytes_col(x) -> np.ndarray:
    """a byte column as the C ABI wants it, without copying arrays that already are one (pinned buffers stay pinned)"""
    if isinstance(x, np.ndarray) and x.dtype == np.uint8 and x.flags["C_CONTIGUOUS"] and x.size:
        return x.reshape(-1)
    return np.frombuffer(bytes(x) or b"\0", dtype=np.uint8)


def proposal_columns(raws, rounds):
    """the proposals of a batch as the C ABI wants them: `raws` is a list of bytes-likes or a pair (raw, raw_off) — the concatenated
    bytes (bytes or a uint8 array; a pinned one stays pinned) and n + 1 offsets — → (raw uint8[], raw_off uint32[n + 1], round uint64[n])"""
    if isinstance(raws, tuple) and len(raws) == 2 and not isinstance(raws[1], (bytes, bytearray, memoryview)):
        raw, off = _bytes_col(raws[0]), np.ascontiguousarray(raws[1], dtype=np.uint32)
    else:
        raws = [bytes(r) for r in raws]
        raw = _bytes_col(b"".join(raws))
        off = np.zeros(len(raws) + 1, dtype=np.uint32)
        total = np.cumsum([len(r) for r in raws], dtype=np.uint64)
        if len(total) and int(total[-1]) > 0xFFFFFFFF:
            raise ValueError("proposals of one call must stay below 4 GiB (32-bit offsets)")
        off[1:] = total
    rnd = np.ascontiguousarray(rounds, dtype=np.uint64).reshape(-1)
    if len(off) != len(rnd) + 1:
        raise ValueError("raw_off needs one entry more than there are rounds")
    return raw, off, rnd


def shard_range(n_total: int, rank: int, world: int) -> tuple[int, int]:
    """ibft_shard_range (pure): rows [lo, hi) of rank `rank`"""
    lo, hi = C.c_uint64(), C.c_uint64()
    rc = load_library().ibft_shard_range(n_total, rank, world, C.byref(lo), C.byref(hi))
    if rc:
        raise ValueError(f"ibft_shard_range: {rc}")
    return lo.value, hi.value


def exchange_layout(n_total: int, world: int, n_validators: int, n_masks: int = 1) -> tuple[int, int, int]:
    """ibft_exchange_layout (pure): (verdict words per rank, bitmap words per rank, u64 slots of the exchange buffer)"""
    w, b, s = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = load_library().ibft_exchange_layout(n_total, world, n_validators, n_masks, C.byref(w), C.byref(b), C.byref(s))
    if rc:
        raise ValueError(f"ibft_exchange_layout: {rc}")
    return w.value, b.value, s.value


def keccak256(a: bytes, b: bytes = b"") -> bytes:
    """ibft_keccak256: keccak256(a ‖ b) by the library's host routine (no device needed)"""
    a, b = bytes(a), bytes(b)
    out = C.create_string_buffer(32)
    rc = load_library().ibft_keccak256(a or None, len(a), b or None, len(b), out)
    if rc:
        raise ValueError(f"ibft_keccak256: {rc}")
    return out.raw


def comm_preload() -> None:
    """ibft_comm_preload: map librccl now (before anything else in the process maps another copy under the same SONAME)"""
    rc = load_library().ibft_comm_preload()
    if rc != 0:
        raise GpuUnavailable(f"ibft_comm_preload: {load_library().ibft_strerror(rc).decode()} ({rc})")


def comm_unique_id() -> bytes:
    """ibft_comm_unique_id: rank 0 creates it and hands it to the other ranks (loads librccl)"""
    buf = np.zeros(COMM_ID_BYTES, dtype=np.uint8)
    L = load_library()
    rc = L.ibft_comm_unique_id(_p(buf))
    if rc:
        raise GpuUnavailable(f"ibft_comm_unique_id: {L.ibft_strerror(rc).decode()} ({rc})")
    return buf.tobytes()


def _u8(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a.reshape(shape) if shape is not None else a


def mask_to_bool(mask: np.ndarray, n: int) -> np.ndarray:
    bits = np.unpackbits(mask.view(np.uint8), bitorder="little")
    return bits[:n].astype(bool)


def bool_to_mask(v: np.ndarray) -> np.ndarray:
    n = len(v)
    words = (n + 63) // 64
    bits = np.zeros(words * 64, dtype=np.uint8)
    bits[:n] = np.asarray(v, dtype=np.uint8)
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


class BatchVerifier:
    """One ibft_ctx: one HIP stream + resident columns on one MI355X."""

    def __init__(self, device: int = 0, flags: int = 0, max_rows: int = 65536, kernel: int = KERNEL_AUTO):
        self._L = load_library()
        self._h = C.c_void_p()
        cfg = Cfg(device, flags, max_rows, kernel)
        rc = self._L.ibft_ctx_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise GpuUnavailable(f"ibft_ctx_create: {self._L.ibft_strerror(rc).decode()} ({rc})")
        self.max_rows = max_rows
        self._block_cols = []   # the arrays of the streamed block batches in flight, oldest first (kept alive until their collect)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.ibft_ctx_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _chk(self, rc: int, what: str):
        if rc != 0:
            detail = self._L.ibft_last_error(self._h).decode()
            raise RuntimeError(f"{what}: {self._L.ibft_strerror(rc).decode()} ({rc}) {detail}")

    # ValidatorBackend.GetVotingPowers -> device table
    def set_validators(self, height: int, addrs20, power) -> None:
        a = _u8(addrs20, (-1, 20)); p = np.ascontiguousarray(power, dtype=np.uint64)
        assert len(a) == len(p)
        self._chk(self._L.ibft_set_validators(self._h, height, _p(a), _p(p), len(p)), "ibft_set_validators")

    def set_validators_u256(self, height: int, addrs20, powers) -> None:
        """powers: Python ints < 2^256 (GetVotingPowers' *big.Int values)"""
        a = _u8(addrs20, (-1, 20)); p = powers_be32(powers)
        assert len(a) == len(p)
        self._chk(self._L.ibft_set_validators_u256(self._h, height, _p(a), _p(p), len(p)), "ibft_set_validators_u256")

    def last_tally_wide(self) -> TallyWide:
        t = TallyWide()
        self._chk(self._L.ibft_last_tally_wide(self._h, C.byref(t)), "ibft_last_tally_wide")
        return t

    def set_seal_digest(self, suffix: bytes | None) -> None:
        """the embedding Backend's seal convention: None = the seal signs the proposalHash itself (default),
        bytes = it signs keccak256(proposalHash ‖ suffix)  (include/ibftgpu.h: ibft_set_seal_digest)"""
        b = None if not suffix else np.frombuffer(bytes(suffix), dtype=np.uint8)
        self._chk(self._L.ibft_set_seal_digest(self._h, 0 if suffix is None else 1, _p(b), len(suffix or b"")),
                  "ibft_set_seal_digest")
        self._staged = 0

    def try_set_validators(self, height: int, addrs20, power) -> int:
        a = _u8(addrs20, (-1, 20)); p = np.ascontiguousarray(power, dtype=np.uint64)
        return self._L.ibft_set_validators(self._h, height, _p(a), _p(p), len(p))

    def proposal_hash(self, raw: bytes, round_: int) -> bytes:
        out = np.zeros(32, dtype=np.uint8)
        r = np.frombuffer(bytes(raw) or b"\0", dtype=np.uint8)
        self._chk(self._L.ibft_proposal_hash(self._h, _p(r), len(raw), round_, _p(out)), "ibft_proposal_hash")
        return out.tobytes()

    # Verifier.IsValidProposalHash, batched
    def is_valid_proposal_hash(self, raw: bytes, round_: int, hash32, hash_len) -> np.ndarray:
        h = _u8(hash32, (-1, 32)); hl = _u8(hash_len)
        n = len(hl)
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        r = np.frombuffer(bytes(raw) or b"\0", dtype=np.uint8)
        self._chk(self._L.ibft_verify_hashes(self._h, _p(r), len(raw), round_, _p(h), _p(hl), n, _p(mask)),
                  "ibft_verify_hashes")
        return mask_to_bool(mask, n)

    def is_valid_proposal_hash_digest(self, digest32: bytes, hash32, hash_len) -> np.ndarray:
        """IsValidProposalHash with keccak(proposal) already known to the caller: a compare per row"""
        h = _u8(hash32, (-1, 32)); hl = _u8(hash_len)
        n = len(hl)
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        d = np.frombuffer(bytes(digest32), dtype=np.uint8).copy()
        assert len(d) == 32
        self._chk(self._L.ibft_verify_hashes_digest(self._h, _p(d), _p(h), _p(hl), n, _p(mask)), "ibft_verify_hashes_digest")
        return mask_to_bool(mask, n)

    # Verifier.IsValidCommittedSeal, batched
    def is_valid_committed_seal(self, hash32, sig65, signer20, pre_flags=None):
        h = _u8(hash32, (-1, 32)); s = _u8(sig65, (-1, 65)); f = _u8(signer20, (-1, 20))
        n = len(s)
        pre = None if pre_flags is None else _u8(pre_flags)
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        self._chk(self._L.ibft_verify_seals(self._h, _p(h), _p(s), _p(f), _p(pre), n, _p(mask), C.byref(t)),
                  "ibft_verify_seals")
        return mask_to_bool(mask, n), t

    # chain sync: IsValidCommittedSeal + HasQuorum for many finalized blocks in one call
    def _need(self, name: str):
        if not hasattr(self._L, name):
            raise GpuUnavailable(f"this build of the library has no {name} — rebuild")

    @staticmethod
    def _block_columns(seal_off, sig65, pre_flags, *, hashes=None, proposals=None, signer20=None, bare=False, block_set=None):
        """the columns of a block batch as the C ABI wants them, lengths checked → (front, back, n, n_blocks): the columns every
        block call takes in front of n_blocks — the head: (block_hash32,) from `hashes`, or (raw, raw_off, round) from `proposals`
        = (raws, rounds); seal_off; the uint32 block_set column of a _sets call, one entry per block — and behind it — sig65,
        signer20 unless the seals are `bare`, pre_flags (None as given)"""
        head = None if proposals is None else proposal_columns(*proposals)
        off = np.ascontiguousarray(seal_off, dtype=np.uint32)
        nb = len(off) - 1
        if nb < 0:
            raise ValueError("seal_off needs n_blocks + 1 entries")
        if head is None:
            head = (_u8(hashes, (-1, 32)),)
        s = _u8(sig65, (-1, 65))
        f = None if bare else _u8(signer20, (-1, 20))
        n = len(s)
        if (len(head[-1]) != nb or (block_set is not None and len(block_set) != nb) or (f is not None and len(f) != n)
                or int(off[-1]) != n):
            what = ("one proposal per block" if proposals is not None else
                    "block_hash32 / block_set need one row per block" if block_set is not None else
                    "block_hash32 needs one row per block")
            raise ValueError(what + ", seal_off[-1] the number of seals")
        pre = None if pre_flags is None else _u8(pre_flags)
        return [*head, off, *([] if block_set is None else [block_set])], [s, *([] if bare else [f]), pre], n, nb

    def _block_args(self, name, seal_off, sig65, pre_flags, **kind):
        """what every block call starts with: the export is there, the columns are in order → (columns, C arguments, n, n_blocks)"""
        self._need(name)
        if "block_set" in kind:   # (a _sets call)
            kind["block_set"] = np.ascontiguousarray(kind["block_set"], dtype=np.uint32)
        front, back, n, nb = self._block_columns(seal_off, sig65, pre_flags, **kind)
        return front + back, [self._h, *map(_p, front), nb, *map(_p, back)], n, nb

    def _block_call(self, name, seal_off, sig65, pre_flags, *, want_hashes=False, **kind):
        """one of the eight synchronous block calls → (signer20, vidx — the recover calls —, verdict bool[n], Tally list[n_blocks],
        block_hash32 or None — the _raw calls)"""
        bare, raw = kind.get("bare", False), "proposals" in kind
        _, args, n, nb = self._block_args(name, seal_off, sig65, pre_flags, **kind)
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        tallies = (Tally * max(nb, 1))()
        signer = np.zeros((max(n, 1), 20), dtype=np.uint8) if bare else None
        vidx = np.full(max(n, 1), -1, dtype=np.int32) if bare else None
        bh = np.zeros((max(nb, 1), 32), dtype=np.uint8) if want_hashes else None
        outs = ([_p(bh)] if raw else []) + ([_p(signer), _p(vidx)] if bare else []) + [_p(mask), tallies]
        self._chk(getattr(self._L, name)(*args, *outs), name)
        # the rows stay the resident batch of a verify call under the one set; bare rows and rows judged under a family do not
        self._staged = 0 if bare or "block_set" in kind else n
        out = ((signer[:n], vidx[:n]) if bare else ()) + (mask_to_bool(mask, n), list(tallies)[:nb])
        return out + ((bh[:nb] if want_hashes else None,) if raw else ())

    def _block_submit(self, name, seal_off, sig65, pre_flags, **kind) -> int:
        """one of the eight streamed submits: columns checked, the call made, the arrays kept alive until the collect → n"""
        cols, args, n, _ = self._block_args(name, seal_off, sig65, pre_flags, **kind)
        self._chk(getattr(self._L, name)(*args), name)
        self._block_cols.append(tuple(cols))
        if n:   # (as after the synchronous sibling; a batch without rows leaves the resident batch alone)
            self._staged = 0 if kind.get("bare") or "block_set" in kind else n
        return n

    def verify_block_seals(self, block_hash32, seal_off, sig65, signer20, pre_flags=None):
        """ibft_verify_block_seals: block b's seals are rows [seal_off[b], seal_off[b+1]) and sign block_hash32[b] →
        (verdict bool[n], Tally array[n_blocks]) — what one is_valid_committed_seal call per block returns"""
        return self._block_call("ibft_verify_block_seals", seal_off, sig65, pre_flags, hashes=block_hash32, signer20=signer20)

    # bare seals (headers that carry only signatures): who signed?
    def recover_seals(self, hash32, sig65, pre_flags=None):
        """ibft_recover_seals: ecrecover in batch → (signer20 (n, 20) uint8 — zeros where nothing is recovered —, vidx int32[n]
        — index in the validator set or -1 —, verdict bool[n] — recovered and a member —, Tally over the distinct members)"""
        self._need("ibft_recover_seals")
        h = _u8(hash32, (-1, 32)); s = _u8(sig65, (-1, 65))
        n = len(s)
        if len(h) != n:
            raise ValueError("hash32 needs one row per seal")
        pre = None if pre_flags is None else _u8(pre_flags)
        signer = np.zeros((max(n, 1), 20), dtype=np.uint8)
        vidx = np.full(max(n, 1), -1, dtype=np.int32)
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        self._chk(self._L.ibft_recover_seals(self._h, _p(h), _p(s), _p(pre), n, _p(signer), _p(vidx), _p(mask), C.byref(t)),
                  "ibft_recover_seals")
        self._staged = 0
        return signer[:n], vidx[:n], mask_to_bool(mask, n), t

    def recover_block_seals(self, block_hash32, seal_off, sig65, pre_flags=None):
        """ibft_recover_block_seals: recover_seals for many finalized blocks in one call (rows and offsets as
        verify_block_seals, no signer column) → (signer20 (n, 20), vidx int32[n], verdict bool[n], Tally list[n_blocks])"""
        return self._block_call("ibft_recover_block_seals", seal_off, sig65, pre_flags, hashes=block_hash32, bare=True)

    # chain sync across validator-set changes: a family of sets on the context, a set per block
    @staticmethod
    def _set_columns(sets, u256: bool):
        """sets: a list of (addrs20, powers) or (height, addrs20, powers) → (heights u64[n_sets], set_off u32[n_sets + 1],
        addrs (total, 20) u8, powers)"""
        heights, off, addrs, powers = [], [0], [], []
        for k, st in enumerate(sets):
            h, a, p = st if len(st) == 3 else (k, st[0], st[1])
            a = _u8(a, (-1, 20))
            p = powers_be32(p) if u256 else np.ascontiguousarray(p, dtype=np.uint64)
            if len(a) != len(p):
                raise ValueError("a set needs one power per address")
            heights.append(int(h)); off.append(off[-1] + len(a)); addrs.append(a); powers.append(p)
        a = np.concatenate(addrs) if addrs else np.zeros((0, 20), dtype=np.uint8)
        p = np.concatenate(powers) if powers else np.zeros((0, 32) if u256 else 0, dtype=np.uint8 if u256 else np.uint64)
        return (np.asarray(heights, dtype=np.uint64), np.asarray(off, dtype=np.uint32), np.ascontiguousarray(a),
                np.ascontiguousarray(p))

    def try_set_validator_sets(self, sets, u256: bool = False) -> int:
        name = "ibft_set_validator_sets_u256" if u256 else "ibft_set_validator_sets"
        self._need(name)
        h, off, a, p = self._set_columns(sets, u256)
        return getattr(self._L, name)(self._h, len(h), _p(h), _p(off), _p(a) if len(a) else None, _p(p) if len(p) else None)

    def set_validator_sets(self, sets) -> None:
        """ibft_set_validator_sets: install a family of validator sets — a list of (addrs20, powers) or (height, addrs20,
        powers) — next to the single set of set_validators; block b of a _sets call names its set by its index here"""
        self._chk(self.try_set_validator_sets(sets, False), "ibft_set_validator_sets")

    def set_validator_sets_u256(self, sets) -> None:
        """the same with powers as Python ints < 2^256"""
        self._chk(self.try_set_validator_sets(sets, True), "ibft_set_validator_sets_u256")

    def validator_sets_info(self):
        """→ (sets, union addresses, device bytes) of the installed family; (0, 0, 0) without one"""
        self._need("ibft_validator_sets_info")
        n, u, b = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._chk(self._L.ibft_validator_sets_info(self._h, C.byref(n), C.byref(u), C.byref(b)), "ibft_validator_sets_info")
        return n.value, u.value, b.value

    def verify_block_seals_sets(self, block_hash32, seal_off, block_set, sig65, signer20, pre_flags=None):
        """ibft_verify_block_seals_sets: verify_block_seals with block b judged under set block_set[b] of the installed family
        → (verdict bool[n], Tally list[n_blocks]; quorum is the block's set's)"""
        return self._block_call("ibft_verify_block_seals_sets", seal_off, sig65, pre_flags, hashes=block_hash32, signer20=signer20,
                                block_set=block_set)

    def recover_block_seals_sets(self, block_hash32, seal_off, block_set, sig65, pre_flags=None):
        """ibft_recover_block_seals_sets: recover_block_seals with a set per block → (signer20 (n, 20), vidx int32[n] — the index
        in the BLOCK's set or -1 —, verdict bool[n], Tally list[n_blocks])"""
        return self._block_call("ibft_recover_block_seals_sets", seal_off, sig65, pre_flags, hashes=block_hash32, bare=True,
                                block_set=block_set)

    # chain sync from the proposals: the blocks' hashes are computed on the device
    def proposal_hashes(self, raws, rounds) -> np.ndarray:
        """ibft_proposal_hashes: keccak256(raw_i ‖ BE64(round_i)) of n proposals in one call → uint8 (n, 32).  raws: a list of
        bytes, or (raw, raw_off) — see proposal_columns"""
        self._need("ibft_proposal_hashes")
        raw, off, rnd = proposal_columns(raws, rounds)
        n = len(rnd)
        out = np.zeros((max(n, 1), 32), dtype=np.uint8)
        self._chk(self._L.ibft_proposal_hashes(self._h, _p(raw), _p(off), _p(rnd), n, _p(out)), "ibft_proposal_hashes")
        return out[:n]

    def verify_block_seals_raw(self, raws, rounds, seal_off, sig65, signer20, pre_flags=None, want_hashes: bool = True):
        """ibft_verify_block_seals_raw: verify_block_seals with the blocks' PROPOSALS (raws, rounds as for proposal_hashes) in
        place of their hashes → (verdict bool[n], Tally list[n_blocks], block_hash32 (n_blocks, 32) or None)"""
        return self._block_call("ibft_verify_block_seals_raw", seal_off, sig65, pre_flags, proposals=(raws, rounds), signer20=signer20,
                                want_hashes=want_hashes)

    def recover_block_seals_raw(self, raws, rounds, seal_off, sig65, pre_flags=None, want_hashes: bool = True):
        """ibft_recover_block_seals_raw: recover_block_seals with the blocks' PROPOSALS in place of their hashes →
        (signer20 (n, 20), vidx int32[n], verdict bool[n], Tally list[n_blocks], block_hash32 (n_blocks, 32) or None)"""
        return self._block_call("ibft_recover_block_seals_raw", seal_off, sig65, pre_flags, proposals=(raws, rounds), bare=True,
                                want_hashes=want_hashes)

    # chain sync as a stream: submit(k + 1), collect(k) — at most two batches in flight
    def _need_block_stream(self):
        for name in ("ibft_block_seals_submit", "ibft_block_seals_collect", "ibft_block_seals_pending"):
            if not hasattr(self._L, name):
                raise GpuUnavailable(f"this build of the library has no {name} — rebuild")

    def block_seals_submit(self, block_hash32, seal_off, sig65, signer20, pre_flags=None) -> int:
        """ibft_block_seals_submit: the batch of verify_block_seals, enqueued and not waited for → its row count.  The arrays
        are kept alive here until the batch is collected; pass ibft_pinned_alloc memory — pinned_copy() — for the copy to
        run under the kernels of the batch before."""
        self._need_block_stream()
        n = self._block_submit("ibft_block_seals_submit", seal_off, sig65, pre_flags, hashes=block_hash32, signer20=signer20)
        self._staged = n   # this one — the oldest submit — says so even for a batch without rows; its seven siblings only when n > 0
        return n

    def block_seals_collect(self):
        """ibft_block_seals_collect: the OLDEST submitted batch → (verdict bool[n], Tally list[n_blocks]), what
        verify_block_seals returns for it; waits for that batch only"""
        self._need_block_stream()
        _, n, nb = self.block_seals_pending()     # the library's own counts size the buffers
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        tallies = (Tally * max(nb, 1))()
        self._chk(self._L.ibft_block_seals_collect(self._h, _p(mask), tallies), "ibft_block_seals_collect")
        if self._block_cols:
            self._block_cols.pop(0)
        return mask_to_bool(mask, n), list(tallies)[:nb]

    def block_seals_pending(self):
        """ibft_block_seals_pending: (batches in flight, rows of the oldest, blocks of the oldest)"""
        self._need_block_stream()
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.ibft_block_seals_pending(self._h, C.byref(a), C.byref(b), C.byref(c)), "ibft_block_seals_pending")
        return int(a.value), int(b.value), int(c.value)

    # … from the proposals and from bare seals: the same two slots, collected with block_seals_collect_ex
    BATCH_RECOVER, BATCH_RAW, BATCH_SETS = 1, 2, 4   # IBFT_BATCH_*: the kind bits of a batch in flight

    def block_seals_submit_raw(self, raws, rounds, seal_off, sig65, signer20, pre_flags=None) -> int:
        """ibft_block_seals_submit_raw: the batch of verify_block_seals_raw, enqueued and not waited for → its row count.
        The arrays (the proposal bytes included) are kept alive here until the batch is collected."""
        return self._block_submit("ibft_block_seals_submit_raw", seal_off, sig65, pre_flags, proposals=(raws, rounds), signer20=signer20)

    def recover_block_seals_submit(self, block_hash32, seal_off, sig65, pre_flags=None) -> int:
        """ibft_recover_block_seals_submit: the batch of recover_block_seals, enqueued and not waited for → its row count"""
        return self._block_submit("ibft_recover_block_seals_submit", seal_off, sig65, pre_flags, hashes=block_hash32, bare=True)

    def recover_block_seals_submit_raw(self, raws, rounds, seal_off, sig65, pre_flags=None) -> int:
        """ibft_recover_block_seals_submit_raw: the batch of recover_block_seals_raw, enqueued and not waited for → its row count"""
        return self._block_submit("ibft_recover_block_seals_submit_raw", seal_off, sig65, pre_flags, proposals=(raws, rounds), bare=True)

    def block_seals_collect_ex(self) -> dict:
        """ibft_block_seals_collect_ex: the OLDEST submitted batch of any kind → a dict with what its kind carries: always
        "kind", "verdict" (bool[n]) and "tallies" (Tally list[n_blocks]); "block_hash32" (n_blocks, 32) for a batch submitted
        raw; "signer20" (n, 20) and "vidx" (int32[n]) for a recover batch.  Buffers are sized from block_seals_pending_ex."""
        self._need("ibft_block_seals_collect_ex")
        _, n, nb, kind = self.block_seals_pending_ex()
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        tallies = (Tally * max(nb, 1))()
        bh = np.zeros((max(nb, 1), 32), dtype=np.uint8) if kind & self.BATCH_RAW else None
        signer = np.zeros((max(n, 1), 20), dtype=np.uint8) if kind & self.BATCH_RECOVER else None
        vidx = np.full(max(n, 1), -1, dtype=np.int32) if kind & self.BATCH_RECOVER else None
        self._chk(self._L.ibft_block_seals_collect_ex(self._h, _p(bh), _p(signer), _p(vidx), _p(mask), tallies),
                  "ibft_block_seals_collect_ex")
        if self._block_cols:
            self._block_cols.pop(0)
        out = {"kind": kind, "verdict": mask_to_bool(mask, n), "tallies": list(tallies)[:nb]}
        if bh is not None:
            out["block_hash32"] = bh[:nb]
        if signer is not None:
            out["signer20"] = signer[:n]
            out["vidx"] = vidx[:n]
        return out

    def block_seals_pending_ex(self):
        """ibft_block_seals_pending_ex: (batches in flight, rows, blocks and kind — BATCH_* bits — of the oldest)"""
        self._need("ibft_block_seals_pending_ex")
        a, b, c, k = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.ibft_block_seals_pending_ex(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(k)),
                  "ibft_block_seals_pending_ex")
        return int(a.value), int(b.value), int(c.value), int(k.value)

    # … and under a family of sets, a set per block: the _sets calls from the proposals, and all four as a stream
    def verify_block_seals_sets_raw(self, raws, rounds, seal_off, block_set, sig65, signer20, pre_flags=None, want_hashes: bool = True):
        """ibft_verify_block_seals_sets_raw: verify_block_seals_sets with the blocks' PROPOSALS in place of their hashes →
        (verdict bool[n], Tally list[n_blocks], block_hash32 (n_blocks, 32) or None)"""
        return self._block_call("ibft_verify_block_seals_sets_raw", seal_off, sig65, pre_flags, proposals=(raws, rounds),
                                signer20=signer20, block_set=block_set, want_hashes=want_hashes)

    def recover_block_seals_sets_raw(self, raws, rounds, seal_off, block_set, sig65, pre_flags=None, want_hashes: bool = True):
        """ibft_recover_block_seals_sets_raw: recover_block_seals_sets with the blocks' PROPOSALS in place of their hashes →
        (signer20 (n, 20), vidx int32[n], verdict bool[n], Tally list[n_blocks], block_hash32 (n_blocks, 32) or None)"""
        return self._block_call("ibft_recover_block_seals_sets_raw", seal_off, sig65, pre_flags, proposals=(raws, rounds), bare=True,
                                block_set=block_set, want_hashes=want_hashes)

    def block_seals_submit_sets(self, block_hash32, seal_off, block_set, sig65, signer20, pre_flags=None) -> int:
        """ibft_block_seals_submit_sets: the batch of verify_block_seals_sets, enqueued and not waited for → its row count.
        Judged under the family installed NOW, whatever is installed before its collect (block_seals_collect[_ex])."""
        return self._block_submit("ibft_block_seals_submit_sets", seal_off, sig65, pre_flags, hashes=block_hash32, signer20=signer20,
                                  block_set=block_set)

    def block_seals_submit_sets_raw(self, raws, rounds, seal_off, block_set, sig65, signer20, pre_flags=None) -> int:
        """ibft_block_seals_submit_sets_raw: the batch of verify_block_seals_sets_raw, enqueued and not waited for → its row count"""
        return self._block_submit("ibft_block_seals_submit_sets_raw", seal_off, sig65, pre_flags, proposals=(raws, rounds),
                                  signer20=signer20, block_set=block_set)

    def recover_block_seals_submit_sets(self, block_hash32, seal_off, block_set, sig65, pre_flags=None) -> int:
        """ibft_recover_block_seals_submit_sets: the batch of recover_block_seals_sets, enqueued and not waited for → its row count"""
        return self._block_submit("ibft_recover_block_seals_submit_sets", seal_off, sig65, pre_flags, hashes=block_hash32, bare=True,
                                  block_set=block_set)

    def recover_block_seals_submit_sets_raw(self, raws, rounds, seal_off, block_set, sig65, pre_flags=None) -> int:
        """ibft_recover_block_seals_submit_sets_raw: the batch of recover_block_seals_sets_raw, enqueued and not waited for → its
        row count"""
        return self._block_submit("ibft_recover_block_seals_submit_sets_raw", seal_off, sig65, pre_flags, proposals=(raws, rounds),
                                  bare=True, block_set=block_set)

    # Verifier.IsValidValidator, batched
    def is_valid_validator(self, payload: bytes, off, sig65, from20, pre_flags=None):
        pl = _bytes_col(payload)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        s = _u8(sig65, (-1, 65)); f = _u8(from20, (-1, 20))
        n = len(s)
        pre = None if pre_flags is None else _u8(pre_flags)
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        self._chk(self._L.ibft_verify_senders(self._h, _p(pl), _p(off), _p(s), _p(f), _p(pre), n, _p(mask),
                                              C.byref(t)), "ibft_verify_senders")
        return mask_to_bool(mask, n), t

    # a whole PREPARE / COMMIT set in one call: IsValidValidator ∧ IsValidProposalHash (∧ IsValidCommittedSeal)
    def verify_messages(self, payload: bytes, off, msg_sig65, from20, hash32, hash_len, seal65=None, sender_pre=None, valid_pre=None,
                        raw: bytes | None = None, round_: int = 0, digest32: bytes | None = None, proposer: bytes | None = None):
        """→ (sender bool[n], valid bool[n], Tally over sender ∧ valid); seal65=None for a PREPARE set; proposer (20 bytes):
        the tally is ValidatorManager.HasPrepareQuorum with that proposer instead of HasQuorum"""
        pr = None if proposer is None else np.frombuffer(bytes(proposer), dtype=np.uint8)
        pl = _bytes_col(payload)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        s = _u8(msg_sig65, (-1, 65)); f = _u8(from20, (-1, 20)); h = _u8(hash32, (-1, 32)); hl = _u8(hash_len)
        n = len(s)
        sl = None if seal65 is None else _u8(seal65, (-1, 65))
        spre = None if sender_pre is None else _u8(sender_pre)
        vpre = None if valid_pre is None else _u8(valid_pre)
        rawb = None if raw is None else np.frombuffer(bytes(raw) or b"\0", dtype=np.uint8)
        dg = None if digest32 is None else np.frombuffer(bytes(digest32), dtype=np.uint8)
        ms = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        mv = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        self._chk(self._L.ibft_verify_messages(self._h, _p(pl), _p(off), _p(s), _p(f), _p(h), _p(hl), _p(sl), _p(spre), _p(vpre), n,
                                               _p(rawb), 0 if raw is None else len(raw), round_, _p(dg), _p(pr), _p(ms), _p(mv),
                                               C.byref(t)), "ibft_verify_messages")
        return mask_to_bool(ms, n), mask_to_bool(mv, n), t

    def prepare_messages(self, payload, off, msg_sig65, from20, hash32, hash_len, seal65=None, sender_pre=None, valid_pre=None,
                         raw: bytes | None = None, round_: int = 0, digest32: bytes | None = None, proposer: bytes | None = None):
        """verify_messages with the argument marshalling done ONCE: for a caller whose columns live in fixed buffers that
        are refilled every round (what the integration prescribes).  Returns run() → (sender words u64[⌈n/64⌉], valid words,
        Tally); the word arrays are reused between calls.  Decode with mask_to_bool(words, n)."""
        pl = _bytes_col(payload)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        s = _u8(msg_sig65, (-1, 65)); f = _u8(from20, (-1, 20)); h = _u8(hash32, (-1, 32)); hl = _u8(hash_len)
        n = len(s)
        sl = None if seal65 is None else _u8(seal65, (-1, 65))
        spre = None if sender_pre is None else _u8(sender_pre)
        vpre = None if valid_pre is None else _u8(valid_pre)
        rawb = None if raw is None else np.frombuffer(bytes(raw) or b"\0", dtype=np.uint8)
        dg = None if digest32 is None else np.frombuffer(bytes(digest32), dtype=np.uint8)
        ms = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        mv = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        pr = None if proposer is None else np.frombuffer(bytes(proposer), dtype=np.uint8)
        keep = (pl, off, s, f, h, hl, sl, spre, vpre, rawb, dg, pr)  # the pointers below stay valid while these live
        args = (self._h, _p(pl), _p(off), _p(s), _p(f), _p(h), _p(hl), _p(sl), _p(spre), _p(vpre), n, _p(rawb),
                0 if raw is None else len(raw), round_, _p(dg), _p(pr), _p(ms), _p(mv), C.byref(t))
        fn, chk = self._L.ibft_verify_messages, self._chk

        def run(_keep=keep):
            chk(fn(*args), "ibft_verify_messages")
            return ms, mv, t
        run.n = n
        return run

    # §8f rank 3: a3 straight from the wire bytes (PREPARE / COMMIT); rows["status"] == WIRE_NEEDS_HOST
    # are not judged (verdict 0) and go through the protobuf runtime + is_valid_validator
    def is_valid_validator_wire(self, wire: bytes, off):
        wb = np.frombuffer(bytes(wire) or b"\0", dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = len(off) - 1
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        rows = np.zeros(n, dtype=WIRE_ROW)
        t = Tally()
        self._chk(self._L.ibft_verify_senders_wire(self._h, _p(wb), _p(off), n, _p(mask), _p(rows) if n else None,
                                                   C.byref(t)), "ibft_verify_senders_wire")
        self._staged = n
        return mask_to_bool(mask, n), rows, t

    # the same under a family of sets: every message judged under the validator set of ITS height
    def try_set_height_sets(self, first_height, range_set) -> int:
        self._need("ibft_set_height_sets")
        fh = np.ascontiguousarray(first_height, dtype=np.uint64)
        rs = np.ascontiguousarray(range_set, dtype=np.uint32)
        if len(rs) and len(fh) != len(rs) + 1:
            raise ValueError("first_height needs one entry more than range_set")
        return self._L.ibft_set_height_sets(self._h, len(rs), _p(fh) if len(rs) else None, _p(rs) if len(rs) else None)

    def set_height_sets(self, first_height, range_set) -> None:
        """ibft_set_height_sets: heights in [first_height[k], first_height[k+1]) are judged under set range_set[k] of the
        installed family; empty lists clear the map.  Installing a family drops the map."""
        self._chk(self.try_set_height_sets(first_height, range_set), "ibft_set_height_sets")

    def height_sets_info(self):
        """→ (ranges, first mapped height, first height past the last range) of the installed map; (0, 0, 0) without one"""
        self._need("ibft_height_sets_info")
        n, lo, hi = C.c_uint32(), C.c_uint64(), C.c_uint64()
        self._chk(self._L.ibft_height_sets_info(self._h, C.byref(n), C.byref(lo), C.byref(hi)), "ibft_height_sets_info")
        return n.value, lo.value, hi.value

    def verify_senders_wire_sets(self, wire, off, want_rows: bool = True):
        """ibft_verify_senders_wire_sets: is_valid_validator_wire for a batch that mixes heights, every message under the set the
        height map names for its height → (verdict bool[n], rows or None, set int32[n] (-1: none), vidx int32[n] — the index in
        the ROW's set or -1 —, Tally list[n_sets])"""
        self._need("ibft_verify_senders_wire_sets")
        wb = _bytes_col(wire)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = len(off) - 1
        ns = self.validator_sets_info()[0]
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        rows = np.zeros(n, dtype=WIRE_ROW) if want_rows else None
        rset = np.full(max(n, 1), -1, dtype=np.int32)
        vidx = np.full(max(n, 1), -1, dtype=np.int32)
        tal = (Tally * max(ns, 1))()
        self._chk(self._L.ibft_verify_senders_wire_sets(self._h, _p(wb), _p(off), n, _p(mask), _p(rows) if (n and want_rows) else None,
                                                        _p(rset), _p(vidx), tal), "ibft_verify_senders_wire_sets")
        self._staged = 0
        return mask_to_bool(mask, n), rows, rset[:n], vidx[:n], [tal[s] for s in range(ns)]

    def verify_senders_wire_views(self, wire, off, views_cap: int, want_rows: bool = True):
        """ibft_verify_senders_wire_views: verify_senders_wire_sets plus one quorum record per (height, round, type, proposal
        hash) with a valid message in the batch → (verdict bool[n], rows or None, set int32[n], vidx int32[n], Tally
        list[n_sets] — byte for byte the sets call's —, view int32[n] (-1: not valid, -2: its view did not fit views_cap),
        stored bool[n] — the rows a Messages store fed the batch in row order still holds —, views WIRE_VIEW[min(n_views,
        views_cap)], n_views)"""
        return self._wire_views("ibft_verify_senders_wire_views", wire, off, views_cap, want_rows, False)

    def verify_messages_wire_views(self, wire, off, views_cap: int, want_rows: bool = True):
        """ibft_verify_messages_wire_views: verify_senders_wire_views with the committed seals of the COMMIT rows judged in the
        same verdict launch → its tuple plus seal bool[n] — the row is valid and its seal recovers to its From over the digest
        of the hash it names.  A COMMIT record has pad[WIRE_VIEW_SEAL_RULE] = 1 and its tally counts the stored rows whose seal
        bit is set."""
        return self._wire_views("ibft_verify_messages_wire_views", wire, off, views_cap, want_rows, True)

    def wire_seal_stats(self):
        """ibft_wire_seal_stats → (commit_rows, seal_rows) of the last verify_messages_wire_views: the COMMIT rows that have a
        set, and the sealable ones — the seal checks the verdict launch was given"""
        self._need("ibft_wire_seal_stats")
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.ibft_wire_seal_stats(self._h, C.byref(a), C.byref(b)), "ibft_wire_seal_stats")
        return a.value, b.value

    def _wire_views(self, name, wire, off, views_cap, want_rows, seals):
        self._need(name)
        wb = _bytes_col(wire)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = len(off) - 1
        ns = self.validator_sets_info()[0]
        cap = min(int(views_cap), n)
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        stored = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        rows = np.zeros(n, dtype=WIRE_ROW) if want_rows else None
        rset = np.full(max(n, 1), -1, dtype=np.int32)
        vidx = np.full(max(n, 1), -1, dtype=np.int32)
        view = np.full(max(n, 1), -1, dtype=np.int32)
        views = np.zeros(max(cap, 1), dtype=WIRE_VIEW)
        nv = C.c_uint32(0)
        tal = (Tally * max(ns, 1))()
        seal = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        args = [self._h, _p(wb), _p(off), n, int(views_cap), _p(mask), _p(rows) if (n and want_rows) else None, _p(rset), _p(vidx), tal,
                _p(view), _p(stored), _p(views), C.byref(nv)] + ([_p(seal)] if seals else [])
        self._chk(getattr(self._L, name)(*args), name)
        self._staged = 0
        out = (mask_to_bool(mask, n), rows, rset[:n], vidx[:n], [tal[s] for s in range(ns)], view[:n], mask_to_bool(stored, n),
               views[:min(nv.value, cap)], nv.value)
        return out + (mask_to_bool(seal, n),) if seals else out

    def verify_messages_wire(self, wire, off, height: int, round_: int, raw: bytes | None = None, proposal_round: int | None = None,
                             digest32: bytes | None = None, want_rows: bool = True, proposer: bytes | None = None):
        """raw messages judged completely → (sender bool[n], valid bool[n], rows or class bytes, Tally): rows = the full
        parse results (want_rows) or the one routing byte per row (CLASS_* bits); see include/ibftgpu.h"""
        wb = _bytes_col(wire)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = len(off) - 1
        ms = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        mv = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        rows = np.zeros(n, dtype=WIRE_ROW) if want_rows else None
        cls = np.zeros(max(n, 1), dtype=np.uint8)
        rawb = None if raw is None else np.frombuffer(bytes(raw) or b"\0", dtype=np.uint8)
        dg = None if digest32 is None else np.frombuffer(bytes(digest32), dtype=np.uint8)
        t = Tally()
        self._chk(self._L.ibft_verify_messages_wire(self._h, _p(wb), _p(off), n, height, round_, _p(rawb),
                                                    0 if raw is None else len(raw),
                                                    round_ if proposal_round is None else proposal_round, _p(dg), _p(ms), _p(mv),
                                                    _p(cls), _p(rows) if (n and want_rows) else None,
                                                    _p(None if proposer is None else np.frombuffer(bytes(proposer), dtype=np.uint8)),
                                                    C.byref(t)),
                  "ibft_verify_messages_wire")
        self._last_class = cls[:n]
        return mask_to_bool(ms, n), mask_to_bool(mv, n), (rows if want_rows else cls[:n]), t

    def verify_certificates_wire(self, wire, off, rows_cap: int | None = None, want_rows: bool = True):
        """§8f rank 2 from bytes: the whole certificate tree of a batch of raw messages →
        (n_rows, nodes[CERT_NODE], rows[WIRE_ROW] or None, class u8[n_rows], sender bool[n_rows], hash bool[n_rows],
        self bool[n_rows]); see include/ibftgpu.h.  Raises RuntimeError (IBFT_E_TOOBIG) when the tree exceeds rows_cap."""
        wb = _bytes_col(wire)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = len(off) - 1
        cap = int(rows_cap if rows_cap is not None else self.max_rows)
        words = (cap + 63) // 64 or 1
        nodes = np.zeros(max(cap, 1), dtype=CERT_NODE)
        rows = np.zeros(max(cap, 1), dtype=WIRE_ROW) if want_rows else None
        cls = np.zeros(max(cap, 1), dtype=np.uint8)
        ms, mh, mself = (np.zeros(words, dtype=np.uint64) for _ in range(3))
        n_rows = C.c_size_t(0)
        self._chk(self._L.ibft_verify_certificates_wire(self._h, _p(wb), _p(off), n, cap, C.byref(n_rows), _p(nodes),
                                                        _p(rows) if want_rows else None, _p(cls), _p(ms), _p(mh), _p(mself)),
                  "ibft_verify_certificates_wire")
        k = int(n_rows.value)
        return (k, nodes[:k], rows[:k] if want_rows else None, cls[:k], mask_to_bool(ms, k), mask_to_bool(mh, k),
                mask_to_bool(mself, k))

    def judge_certificates_wire(self, wire, off, rows_cap: int | None = None, certs_cap: int | None = None, per_row: bool = False):
        """the certificate trees of a batch of raw messages judged PER CARRIER on the device (ibft_judge_certificates_wire):
        → (certs[CERT_VERDICT], n_rows, per_row outputs) — one record per level-0 row and per ROUND_CHANGE message of a root
        PREPREPARE's certificate, with validPC (pc) and the RoundChangeCertificate rules (rcc) decided up to IsProposer; see
        include/ibftgpu.h for how a caller finishes.  per_row: also (nodes, rows, class, sender, hash, self) exactly as
        verify_certificates_wire returns them, else None and nothing per row is copied out.  Raises RuntimeError
        (IBFT_E_TOOBIG) when the tree exceeds rows_cap or the records exceed certs_cap (default: rows_cap)."""
        return _judge_certificates_wire(self._L, self._h, self._chk, wire, off, int(rows_cap if rows_cap is not None else self.max_rows),
                                        certs_cap, per_row)

    def set_proposers(self, height: int, first_round: int, addrs) -> None:
        """the proposer table of decide_certificates_wire (ibft_set_proposers): addrs[k] proposes round first_round + k of
        `height`; it replaces the previous table, an empty addrs clears it.  set_validators leaves it alone."""
        _set_proposers(self._L, self._h, self._chk, height, first_round, addrs)

    def proposers_info(self):
        """(height, first_round, n_rounds) of the installed proposer table; n_rounds == 0: none"""
        return _proposers_info(self._L, self._h, self._chk)

    def decide_certificates_wire(self, wire, off, rows_cap: int | None = None, certs_cap: int | None = None, per_row: bool = False):
        """judge_certificates_wire, and for every record a decision under the proposer table (ibft_decide_certificates_wire):
        → (certs[CERT_VERDICT], decisions[CERT_DECISION], n_rows, per_row outputs) — valid_pc, round_change and proposal are
        −1 (undecided here: no table entry, or an irregular shape), 0 or 1 (valid_pc also 2: no certificate)."""
        return _judge_certificates_wire(self._L, self._h, self._chk, wire, off, int(rows_cap if rows_cap is not None else self.max_rows),
                                        certs_cap, per_row, decide=True)

    def decide_round_changes_wire(self, wire, off, query=None, rows_cap: int | None = None, certs_cap: int | None = None,
                                  rc_cap: int | None = None, per_row: bool = False):
        """decide_certificates_wire, and what handleRoundChangeMessage does with its answers (ibft_decide_round_changes_wire): one
        quorum record per (height, round) of the level-0 ROUND_CHANGE rows and, for `query` (rc_query(...)), GetExtendedRCC /
        GetMostRoundChangeMessages over them → (certs, decisions, n_rows, per_row outputs, (rc_view int32[n], rc_stored bool[n],
        records[RC_RECORD], n_rc, answer[RC_ANSWER] or None)).  rc_cap None: n, which always fits."""
        return _decide_round_changes_wire(self._L, self._h, self._chk, wire, off, query, int(rows_cap if rows_cap is not None else self.max_rows),
                                          certs_cap, rc_cap, per_row)

    def cert_stats(self):
        """ibft_cert_stats, of the last verify_ / judge_certificates_wire call: (rows of the tree, rows judged — no pre-flag —,
        rows given to the verdict kernels, rows the dedup table could not place).  FLAG_CERT_DEDUP off: judged == given, 0."""
        if not hasattr(self._L, "ibft_cert_stats"):
            raise GpuUnavailable("this build of libibftgpu.so has no ibft_cert_stats — rebuild")
        v = [C.c_uint32() for _ in range(4)]
        self._chk(self._L.ibft_cert_stats(self._h, *(C.byref(x) for x in v)), "ibft_cert_stats")
        return tuple(int(x.value) for x in v)

    def wire_stats(self):
        """ibft_wire_stats, of the last is_valid_validator_wire / verify_messages_wire call: (rows, rows judged through the recode
        class — FLAG_WIRE_RECODE; their rows carry pad[0] = 1 —, rows left NEEDS_HOST).  A diagnostic: it copies the parse results."""
        if not hasattr(self._L, "ibft_wire_stats"):
            raise GpuUnavailable("this build of libibftgpu.so has no ibft_wire_stats — rebuild")
        v = [C.c_uint32() for _ in range(3)]
        self._chk(self._L.ibft_wire_stats(self._h, *(C.byref(x) for x in v)), "ibft_wire_stats")
        return tuple(int(x.value) for x in v)

    def wire_stage_seals(self):
        """the COMMIT seals of the last is_valid_validator_wire batch become the resident seal batch"""
        self._chk(self._L.ibft_wire_stage_seals(self._h), "ibft_wire_stage_seals")

    # ValidatorManager.HasQuorum over a caller-supplied verdict array
    def has_quorum(self, sender20, verdict) -> Tally:
        f = _u8(sender20, (-1, 20))
        m = bool_to_mask(np.asarray(verdict, dtype=bool))
        t = Tally()
        self._chk(self._L.ibft_tally(self._h, _p(f), _p(m), len(f), C.byref(t)), "ibft_tally")
        return t

    # ValidatorManager.HasPrepareQuorum (core/validator_manager.go:99-127) over a caller-supplied verdict array
    def has_prepare_quorum(self, sender20, verdict, proposer: bytes) -> Tally:
        f = _u8(sender20, (-1, 20))
        m = bool_to_mask(np.asarray(verdict, dtype=bool))
        pr = np.frombuffer(bytes(proposer), dtype=np.uint8)
        assert len(pr) == 20
        t = Tally()
        self._chk(self._L.ibft_tally_prepare(self._h, _p(f), _p(m), len(f), _p(pr), C.byref(t)), "ibft_tally_prepare")
        return t

    def comm_info(self):
        """(ranks, this rank, device) as the RCCL communicator itself reports them"""
        n, r, d = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        self._chk(self._L.ibft_comm_info(self._h, C.byref(n), C.byref(r), C.byref(d)), "ibft_comm_info")
        return int(n.value), int(r.value), int(d.value)

    # staged / device-resident form of a2 (bench.py, multi-GPU)
    def seals_stage(self, hash32, sig65, signer20, pre_flags=None) -> int:
        h = _u8(hash32, (-1, 32)); s = _u8(sig65, (-1, 65)); f = _u8(signer20, (-1, 20))
        pre = None if pre_flags is None else _u8(pre_flags)
        self._chk(self._L.ibft_seals_stage(self._h, _p(h), _p(s), _p(f), _p(pre), len(s)), "ibft_seals_stage")
        self._staged = len(s)
        return len(s)

    def seals_stage_next(self, hash32, sig65, signer20, pre_flags=None) -> int:
        """the NEXT batch into the spare column set, asynchronously on the context's copy stream (the arrays are kept alive
        here until the swap; pass ibft_pinned_alloc memory — pinned_copy() — for the copy to overlap the kernels)"""
        h = _u8(hash32, (-1, 32)); s = _u8(sig65, (-1, 65)); f = _u8(signer20, (-1, 20))
        pre = None if pre_flags is None else _u8(pre_flags)
        self._next_cols = (h, s, f, pre)
        self._chk(self._L.ibft_seals_stage_next(self._h, _p(h), _p(s), _p(f), _p(pre), len(s)), "ibft_seals_stage_next")
        return len(s)

    def seals_swap(self, wait_for_copy: bool = True) -> None:
        """the staged batch becomes the resident one; per step of a stream: launch(k), stage_next(k+1), fetch(k), swap"""
        self._chk(self._L.ibft_seals_swap(self._h, 1 if wait_for_copy else 0), "ibft_seals_swap")
        self._staged = len(self._next_cols[1])
        self._held_cols, self._next_cols = self._next_cols, None   # (with wait_for_copy=0 the copy may still read them)

    def seals_submit(self) -> None:
        """one more pass over the resident batch, asynchronously (at most two in flight); results through seals_collect"""
        self._chk(self._L.ibft_seals_submit(self._h), "ibft_seals_submit")
        self._submitted = getattr(self, "_submitted", []) + [self._staged]

    def seals_collect(self):
        """the OLDEST submitted pass → (verdict bool[n], Tally); waits for that pass only"""
        n = self._submitted[0] if getattr(self, "_submitted", None) else 0
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        self._chk(self._L.ibft_seals_collect(self._h, _p(mask), C.byref(t)), "ibft_seals_collect")
        self._submitted.pop(0)
        return mask_to_bool(mask, n), t

    def seals_rows(self):
        """ibft_seals_rows: (rows of the resident batch, rows of the oldest submitted pass or 0) as the LIBRARY counts them"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._L.ibft_seals_rows(self._h, C.byref(a), C.byref(b)), "ibft_seals_rows")
        return int(a.value), int(b.value)

    def pipeline_stats(self):
        """ibft_pipeline_stats: (passes whose tally ran on the side stream, batches that went out as two launches)"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        if not hasattr(self._L, "ibft_pipeline_stats"):    # (an older build under IBFT_MIN_ABI: it has no side stream either)
            return 0, 0
        self._chk(self._L.ibft_pipeline_stats(self._h, C.byref(a), C.byref(b)), "ibft_pipeline_stats")
        return int(a.value), int(b.value)

    def alt_verdict_passes(self) -> int:
        """ibft_pipeline_stats_ex: submitted passes whose verdict launch took the second verdict stream"""
        if not hasattr(self._L, "ibft_pipeline_stats_ex"):  # (an older build: it has one verdict stream)
            return 0
        a = C.c_uint32(0)
        self._chk(self._L.ibft_pipeline_stats_ex(self._h, None, None, C.byref(a)), "ibft_pipeline_stats_ex")
        return int(a.value)

    def seals_launch(self, repeat: int = 1) -> None:
        self._chk(self._L.ibft_seals_launch(self._h, repeat), "ibft_seals_launch")
        self._launched = self._staged

    def seals_fetch(self):
        n = getattr(self, "_launched", self._staged)   # the batch of the last launch (a swap may have come in between)
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        self._chk(self._L.ibft_seals_fetch(self._h, _p(mask), C.byref(t)), "ibft_seals_fetch")
        return mask_to_bool(mask, n), t

    def seals_run(self):
        """one more pass over the resident batch (launch + fetch in one C call) → (verdict bool[n], Tally)"""
        n = self._staged
        if getattr(self, "_run_mask", None) is None or len(self._run_mask) != ((n + 63) // 64 or 1):
            self._run_mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        self._chk(self._L.ibft_seals_run(self._h, _p(self._run_mask), C.byref(t)), "ibft_seals_run")
        return mask_to_bool(self._run_mask, n), t

    def _sign_prepare(self, fn_name, nonce, sk32):
        """what every sign_* call starts with: the nonce rule is known, the library has fn_name → (keys u8[n,32], n)"""
        if nonce not in SIGN_NONCES:
            raise ValueError(f"nonce must be one of {sorted(SIGN_NONCES)}, not {nonce!r}")
        if not hasattr(self._L, fn_name):
            raise GpuUnavailable(f"this build of the library has no {fn_name} — rebuild")
        sk = np.ascontiguousarray(sk32, dtype=np.uint8).reshape(-1, 32)
        return sk, len(sk)

    @staticmethod
    def _row_columns(n, *columns):
        """(value, dtype) pairs → contiguous columns of n entries each; a scalar is one value for every row"""
        return [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (n,))) for v, dt in columns]

    def sign_seals(self, sk32, hash32, nonce="keccak"):
        """ibft_sign_seals (simulators only): (sig65 u8[n,65], signer20 u8[n,20], ok bool[n]); leaves the batch staged.
        nonce: "keccak" (the library's own rule, the default) or "rfc6979" (ibft_sign_seals_ex: RFC 6979 §3.2 with
        bits2octets(h1) = h1 mod n — the seals btcec / bitcoinjs produce for the same key and digest)"""
        sk, n = self._sign_prepare("ibft_sign_seals" if nonce == "keccak" else "ibft_sign_seals_ex", nonce, sk32)
        hs = np.ascontiguousarray(hash32, dtype=np.uint8).reshape(-1, 32)
        if len(hs) != n:
            raise ValueError("one hash per key")
        sig = np.zeros((n, 65), dtype=np.uint8)
        signer = np.zeros((n, 20), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        if nonce == "keccak":
            self._chk(self._L.ibft_sign_seals(self._h, _p(sk), _p(hs), n, _p(sig), _p(signer), _p(ok)), "ibft_sign_seals")
        else:
            self._chk(self._L.ibft_sign_seals_ex(self._h, _p(sk), _p(hs), n, SIGN_NONCES[nonce], _p(sig), _p(signer), _p(ok)),
                      "ibft_sign_seals_ex")
        self._staged = n
        return sig, signer, ok.astype(bool)

    def sign_messages(self, sk32, type, height, round, hash32, nonce="keccak"):
        """ibft_sign_messages_wire (simulators only): one PREPARE (type 1) or COMMIT (type 2) message per row, built, hashed,
        signed and encoded on the device → (wire: bytes, off u32[n+1], from20 u8[n,20], ok bool[n]); row i is
        wire[off[i]:off[i+1]], the form is_valid_validator_wire / verify_messages_wire take.  type, height and round are
        columns or scalars (one value for every row).  A COMMIT's seal signs the hash under the context's seal-digest
        convention.  A refused key (ok False) keeps its row's length and carries a zero From, signature and seal.  Leaves no
        staged batch."""
        sk, n = self._sign_prepare("ibft_sign_messages_wire", nonce, sk32)
        hs = np.ascontiguousarray(hash32, dtype=np.uint8).reshape(-1, 32)
        if len(hs) != n:
            raise ValueError("one hash per key")
        ty, hh, rr = self._row_columns(n, (type, np.uint8), (height, np.uint64), (round, np.uint64))
        wire = np.zeros(max(n, 1) * SIGN_MESSAGE_MAX, dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint32)
        frm = np.zeros((n, 20), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        self._chk(self._L.ibft_sign_messages_wire(self._h, _p(sk), _p(ty), _p(hh), _p(rr), _p(hs), n, SIGN_NONCES[nonce], _p(wire),
                                                  wire.size, _p(off), _p(frm), _p(ok)), "ibft_sign_messages_wire")
        self._staged = 0
        return wire[:int(off[n])].tobytes(), off, frm, ok.astype(bool)

    def sign_envelopes(self, sk32, type, height, round, body, body_at, body_len, nonce="keccak"):
        """ibft_sign_envelopes_wire (simulators only): one PREPREPARE (type 0) or ROUND_CHANGE (type 3) message per row around the
        already-encoded body bytes body[body_at[i]:body_at[i] + body_len[i]] — rows may name the same or overlapping ranges —,
        From derived, the envelope hashed and signed on the device → (wire: bytes, off u32[n+1], from20 u8[n,20], ok bool[n]); row i
        is wire[off[i]:off[i+1]], the form verify_certificates_wire takes.  type, height, round, body_at and body_len are columns
        or scalars (one value for every row).  A refused key (ok False) keeps its row's length and carries a zero From and
        signature around its body.  Leaves no staged batch."""
        sk, n = self._sign_prepare("ibft_sign_envelopes_wire", nonce, sk32)
        bb = np.frombuffer(bytes(body), dtype=np.uint8) if not isinstance(body, np.ndarray) else np.ascontiguousarray(body, dtype=np.uint8)
        ty, hh, rr, at, ln = self._row_columns(n, (type, np.uint8), (height, np.uint64), (round, np.uint64), (body_at, np.uint32),
                                               (body_len, np.uint32))
        cap = int(ln.astype(np.uint64).sum()) + ENVELOPE_HEAD_MAX * max(n, 1)
        wire = np.zeros(cap, dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint32)
        frm = np.zeros((n, 20), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.uint8)
        self._chk(self._L.ibft_sign_envelopes_wire(self._h, _p(sk), _p(ty), _p(hh), _p(rr), _p(bb) if bb.size else None, bb.size, _p(at),
                                                   _p(ln), n, SIGN_NONCES[nonce], _p(wire), wire.size, _p(off), _p(frm), _p(ok)),
                  "ibft_sign_envelopes_wire")
        self._staged = 0
        return wire[:int(off[n])].tobytes(), off, frm, ok.astype(bool)

    def forget_proposal(self) -> None:
        """the next call that names a proposal hashes it again (a new height has a new proposal)"""
        self._chk(self._L.ibft_forget_proposal(self._h), "ibft_forget_proposal")

    def gather_batches(self) -> int:
        """batches whose (pinned) columns the device read itself in one gather launch"""
        g = C.c_uint32()
        self._chk(self._L.ibft_column_stats(self._h, C.byref(g)), "ibft_column_stats")
        return g.value

    def seals_device_ptrs(self):
        dm, dt, w = C.c_void_p(), C.c_void_p(), C.c_size_t()
        self._chk(self._L.ibft_seals_device_ptrs(self._h, C.byref(dm), C.byref(w), C.byref(dt)), "device_ptrs")
        return dm.value, w.value, dt.value

    def seals_export(self, d_mask_ptr: int | None, d_tally_ptr: int | None) -> None:
        """D2D copy of mask/tally into caller-owned device memory (torch data_ptr), then sync."""
        self._chk(self._L.ibft_seals_export(self._h, d_mask_ptr, d_tally_ptr), "ibft_seals_export")

    def seals_export_on(self, d_mask_ptr: int | None, d_tally_ptr: int | None, stream: int) -> None:
        """the same copies enqueued on the caller's stream (hipStream_t handle) behind a results-ready event:
        no host wait; the caller's collective overlaps with the next seals_launch"""
        self._chk(self._L.ibft_seals_export_on(self._h, d_mask_ptr, d_tally_ptr, stream), "ibft_seals_export_on")

    # ---- multi-GPU: this context is one rank of a sharded batch (include/ibftgpu.h, ibft_comm_*) ----
    def comm_init(self, unique_id: bytes, rank: int, world: int) -> None:
        uid = np.frombuffer(unique_id, dtype=np.uint8).copy()
        assert len(uid) == COMM_ID_BYTES
        self._chk(self._L.ibft_comm_init(self._h, _p(uid), rank, world), "ibft_comm_init")

    def comm_destroy(self) -> None:
        self._chk(self._L.ibft_comm_destroy(self._h), "ibft_comm_destroy")

    def seals_exchange(self, n_total: int) -> None:
        """enqueue pack + RCCL all-reduce + delivery of the merged result behind the last seals_launch"""
        self._chk(self._L.ibft_seals_exchange(self._h, n_total), "ibft_seals_exchange")
        self._xq = getattr(self, "_xq", [])
        self._xq.append(n_total)

    def seals_fetch_merged(self):
        """oldest outstanding exchange → (global verdict bool[n_total], merged Tally)"""
        n_total = self._xq.pop(0)
        mask = np.zeros((n_total + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        self._chk(self._L.ibft_seals_fetch_merged(self._h, _p(mask), C.byref(t)), "ibft_seals_fetch_merged")
        return mask_to_bool(mask, n_total), t

    def set_kernel_timing(self, every_n: int) -> None:
        """HIP-event pair around the verdict kernels of every n-th staged pass (1 = all, 0 = none)"""
        self._chk(self._L.ibft_set_kernel_timing(self._h, every_n), "ibft_set_kernel_timing")

    def last_kernel_ms(self):
        ms, k = C.c_float(), C.c_uint32()
        self._chk(self._L.ibft_last_kernel_ms(self._h, C.byref(ms), C.byref(k)), "ibft_last_kernel_ms")
        return ms.value, k.value

    def cache_stats(self):
        """(validators with a built table, verdict passes that used the warm kernel, cold passes)."""
        t, w, c, g = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self._L.ibft_cache_stats(self._h, C.byref(t), C.byref(w), C.byref(c), C.byref(g)), "ibft_cache_stats")
        self.lanes_per_signature = g.value
        return t.value, w.value, c.value

    def cache_memory(self):
        """the device-wide key cache: (bytes held, slots in use, slots allocated, contexts sharing it)"""
        b, u, a, k = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self._L.ibft_cache_memory(self._h, C.byref(b), C.byref(u), C.byref(a), C.byref(k)), "ibft_cache_memory")
        return b.value, u.value, a.value, k.value

    def cache_form(self):
        """ibft_cache_form: (table form of the device's key-cache pool — 0 wide, 1 glv: IBFT_QTAB_FORM, read when the first
        context of the device is created —, bytes of one slot's table)"""
        if not hasattr(self._L, "ibft_cache_form"):
            raise GpuUnavailable("this build of libibftgpu.so has no ibft_cache_form — rebuild")
        f, b = C.c_uint32(), C.c_uint64()
        self._chk(self._L.ibft_cache_form(self._h, C.byref(f), C.byref(b)), "ibft_cache_form")
        return f.value, b.value

    def last_dispatch(self):
        """(cold lanes per signature, warm lanes per signature) of the last verdict pass."""
        a, b = C.c_uint32(), C.c_uint32()
        self._chk(self._L.ibft_last_dispatch(self._h, C.byref(a), C.byref(b)), "ibft_last_dispatch")
        return a.value, b.value

    def last_cold_table(self) -> int:
        """where the last lane / group cold kernel kept its window tables: 0 none ran, 1 LDS, 2 private + prefetch, 3 private"""
        t = C.c_uint32()
        self._chk(self._L.ibft_last_cold_table(self._h, C.byref(t)), "ibft_last_cold_table")
        return t.value

    def sync(self):
        self._chk(self._L.ibft_sync(self._h), "ibft_sync")

    def issue_probe(self):
        """ibft_issue_probe: (ns per aligned 8-byte VALU instruction per SIMD at one wavefront per SIMD, ms of the probe
        kernel) — 1.89 ns on a healthy MI355X"""
        ns, ms = C.c_float(0), C.c_float(0)
        self._chk(self._L.ibft_issue_probe(self._h, C.byref(ns), C.byref(ms)), "ibft_issue_probe")
        return float(ns.value), float(ms.value)


class DeviceGroup:
    """ibft_group: one process, several MI355X — rows sharded over the devices, one all-reduce inside the library merges
    verdict words and the ranks' distinct-sender bitmaps (what a Go Backend would call for N beyond one GPU).  A device
    listed several times gives several contexts on that device and the library's own sum kernel as the collective."""

    def __init__(self, devices, flags: int = 0, max_rows_total: int = 0):
        self._L = load_library()
        self._g = C.c_void_p()
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        rc = self._L.ibft_group_create(_p(dv), len(dv), flags, max_rows_total, C.byref(self._g))
        if rc != 0:
            self._g = C.c_void_p()
            raise GpuUnavailable(f"ibft_group_create: {self._L.ibft_strerror(rc).decode()} ({rc})")

    def close(self):
        if getattr(self, "_g", None) and self._g.value:
            self._L.ibft_group_destroy(self._g)
            self._g = C.c_void_p()

    __del__ = close

    def set_seal_digest(self, suffix: bytes | None) -> None:
        b = None if not suffix else np.frombuffer(bytes(suffix), dtype=np.uint8)
        self._chk(self._L.ibft_group_set_seal_digest(self._g, 0 if suffix is None else 1, _p(b), len(suffix or b"")),
                  "ibft_group_set_seal_digest")

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {self._L.ibft_strerror(rc).decode()} ({rc})")

    @property
    def size(self) -> int:
        return self._L.ibft_group_size(self._g)

    def set_validators(self, height: int, addrs20, power) -> None:
        a = _u8(addrs20, (-1, 20)); p = np.ascontiguousarray(power, dtype=np.uint64)
        self._chk(self._L.ibft_group_set_validators(self._g, height, _p(a), _p(p), len(p)), "ibft_group_set_validators")

    def set_validators_u256(self, height: int, addrs20, powers) -> None:
        a = _u8(addrs20, (-1, 20)); p = powers_be32(powers)
        self._chk(self._L.ibft_group_set_validators_u256(self._g, height, _p(a), _p(p), len(p)),
                  "ibft_group_set_validators_u256")

    def is_valid_committed_seal(self, hash32, sig65, signer20, pre_flags=None):
        h = _u8(hash32, (-1, 32)); s = _u8(sig65, (-1, 65)); f = _u8(signer20, (-1, 20))
        n = len(s)
        pre = None if pre_flags is None else _u8(pre_flags)
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        self._chk(self._L.ibft_group_verify_seals(self._g, _p(h), _p(s), _p(f), _p(pre), n, _p(mask), C.byref(t)),
                  "ibft_group_verify_seals")
        return mask_to_bool(mask, n), t

    def is_valid_validator(self, payload: bytes, off, sig65, from20, pre_flags=None):
        pl = _bytes_col(payload)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        s = _u8(sig65, (-1, 65)); f = _u8(from20, (-1, 20))
        n = len(s)
        pre = None if pre_flags is None else _u8(pre_flags)
        mask = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        self._chk(self._L.ibft_group_verify_senders(self._g, _p(pl), _p(off), _p(s), _p(f), _p(pre), n, _p(mask), C.byref(t)),
                  "ibft_group_verify_senders")
        return mask_to_bool(mask, n), t

    def verify_certificates_wire(self, wire, off, rows_cap: int = 65536, want_rows: bool = True):
        """ibft_group_verify_certificates_wire: the trees sharded by carrier over the group's devices, rows numbered as ONE
        call over all messages numbers them; same tuple as BatchVerifier.verify_certificates_wire"""
        wb = _bytes_col(wire)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = len(off) - 1
        cap = int(rows_cap)
        words = (cap + 63) // 64 or 1
        nodes = np.zeros(max(cap, 1), dtype=CERT_NODE)
        rows = np.zeros(max(cap, 1), dtype=WIRE_ROW) if want_rows else None
        cls = np.zeros(max(cap, 1), dtype=np.uint8)
        ms, mh, mself = (np.zeros(words, dtype=np.uint64) for _ in range(3))
        n_rows = C.c_size_t(0)
        self._chk(self._L.ibft_group_verify_certificates_wire(self._g, _p(wb), _p(off), n, cap, C.byref(n_rows), _p(nodes),
                                                              _p(rows) if want_rows else None, _p(cls), _p(ms), _p(mh), _p(mself)),
                  "ibft_group_verify_certificates_wire")
        k = int(n_rows.value)
        return (k, nodes[:k], rows[:k] if want_rows else None, cls[:k], mask_to_bool(ms, k), mask_to_bool(mh, k),
                mask_to_bool(mself, k))

    def judge_certificates_wire(self, wire, off, rows_cap: int = 65536, certs_cap: int | None = None, per_row: bool = False):
        """BatchVerifier.judge_certificates_wire on the group's FIRST context (there is no sharded form of this call: a
        carrier's children must lie on the device that judges it); same results"""
        return _judge_certificates_wire(self._L, self._L.ibft_group_ctx(self._g, 0), self._chk, wire, off, int(rows_cap), certs_cap, per_row)

    def set_proposers(self, height: int, first_round: int, addrs) -> None:
        """BatchVerifier.set_proposers on the group's FIRST context (where decide_certificates_wire runs)"""
        _set_proposers(self._L, self._L.ibft_group_ctx(self._g, 0), self._chk, height, first_round, addrs)

    def proposers_info(self):
        return _proposers_info(self._L, self._L.ibft_group_ctx(self._g, 0), self._chk)

    def decide_certificates_wire(self, wire, off, rows_cap: int = 65536, certs_cap: int | None = None, per_row: bool = False):
        """BatchVerifier.decide_certificates_wire on the group's FIRST context (no sharded form, as for the judge call)"""
        return _judge_certificates_wire(self._L, self._L.ibft_group_ctx(self._g, 0), self._chk, wire, off, int(rows_cap), certs_cap, per_row,
                                        decide=True)

    def decide_round_changes_wire(self, wire, off, query=None, rows_cap: int = 65536, certs_cap: int | None = None, rc_cap: int | None = None,
                                  per_row: bool = False):
        """BatchVerifier.decide_round_changes_wire on the group's FIRST context (no sharded form, as for the decide call)"""
        return _decide_round_changes_wire(self._L, self._L.ibft_group_ctx(self._g, 0), self._chk, wire, off, query, int(rows_cap), certs_cap,
                                          rc_cap, per_row)

    def verify_messages(self, payload: bytes, off, msg_sig65, from20, hash32, hash_len, seal65=None, sender_pre=None,
                        valid_pre=None, raw: bytes | None = None, round_: int = 0, digest32: bytes | None = None,
                        proposer: bytes | None = None):
        """a whole PREPARE / COMMIT set sharded by message → (sender bool[n], valid bool[n], merged Tally)"""
        pr = None if proposer is None else np.frombuffer(bytes(proposer), dtype=np.uint8)
        pl = _bytes_col(payload)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        s = _u8(msg_sig65, (-1, 65)); f = _u8(from20, (-1, 20)); h = _u8(hash32, (-1, 32)); hl = _u8(hash_len)
        n = len(s)
        sl = None if seal65 is None else _u8(seal65, (-1, 65))
        spre = None if sender_pre is None else _u8(sender_pre)
        vpre = None if valid_pre is None else _u8(valid_pre)
        rawb = None if raw is None else np.frombuffer(bytes(raw) or b"\0", dtype=np.uint8)
        dg = None if digest32 is None else np.frombuffer(bytes(digest32), dtype=np.uint8)
        ms = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        mv = np.zeros((n + 63) // 64 or 1, dtype=np.uint64)
        t = Tally()
        self._chk(self._L.ibft_group_verify_messages(self._g, _p(pl), _p(off), _p(s), _p(f), _p(h), _p(hl), _p(sl), _p(spre),
                                                     _p(vpre), n, _p(rawb), 0 if raw is None else len(raw), round_, _p(dg),
                                                     _p(pr), _p(ms), _p(mv), C.byref(t)), "ibft_group_verify_messages")
        return mask_to_bool(ms, n), mask_to_bool(mv, n), t

    @property
    def is_local(self) -> bool:
        """True: the collective is the library's own sum kernel (a device listed more than once), False: RCCL"""
        return self._L.ibft_group_is_local(self._g) == 1

    def last_tally_wide(self) -> TallyWide:
        t = TallyWide()
        self._chk(self._L.ibft_last_tally_wide(self._L.ibft_group_ctx(self._g, 0), C.byref(t)), "ibft_last_tally_wide")
        return t
