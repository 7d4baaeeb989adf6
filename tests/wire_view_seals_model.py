"""A plain model of ibft_verify_messages_wire_views on top of tests/wire_views_model.py: dictionaries and Python integers, no
tables and no device code.

  sealable      a parsed row that may get a seal check: status OK, a set, type 2 with a CommitMessage payload, a 20-byte
                From, a 65-byte seal, a 32-byte proposal hash, From a member of the row's set
  a COMMIT row  status OK, a set, type 2 with a CommitMessage payload (ibft_wire_seal_stats: commit_rows)
  the seal bit  the row is valid (final sender bit), sealable, and its seal recovers — through the CPU oracle's recovery — to
                its From over the digest the seal-digest convention derives from the hash the message carries:
                IsValidCommittedSeal(proposalHash, seal) of core/ibft.go:931-946
  a record      a PREPARE record is the views model's; a COMMIT record (type 2) has pad[0] = 1 and is tallied over the senders
                of the view's stored rows whose seal bit is set — messages.GetValidMessages filters the store, which holds one
                message per sender: a sender whose stored COMMIT has a bad seal counts for nothing
"""
import wire_views_model as VM

E_OK, E_INVAL, E_NOVALSET, E_TOOBIG = VM.E_OK, VM.E_INVAL, VM.E_NOVALSET, VM.E_TOOBIG
PREPARE, COMMIT = VM.PREPARE, VM.COMMIT
KIND_COMMIT = 7          # the oneof field number of CommitMessage
STATUS_OK = 0
SEAL_RULE = 0            # IBFT_WIRE_VIEW_SEAL_RULE

check_call = VM.check_call   # the refusals and their order are the views call's


def seal_digest(h: bytes, suffix, keccak256) -> bytes:
    """ibft_set_seal_digest: identity (suffix None) or keccak256(hash ‖ suffix)"""
    return h if suffix is None else keccak256(h + suffix)


def is_commit(p, s) -> bool:
    """p: an oracle.wire_parse Row, s: the row's set"""
    return p.status == STATUS_OK and s >= 0 and p.type == COMMIT and p.payload_kind == KIND_COMMIT


def is_sealable(p, s, sets) -> bool:
    return (is_commit(p, s) and len(p.sender) == 20 and len(p.committed_seal) == 65 and len(p.proposal_hash) == 32
            and p.sender in sets[s].power)


def seal_bits(parsed, valid, rset, sets, check):
    """check(row number, parsed row) → does the seal recover to From (asked for sealable rows only)
    → (seal [bool], commit_rows, seal_rows, the sealable rows in the order of their seal rows)"""
    dense = [j for j, p in enumerate(parsed) if is_sealable(p, rset[j], sets)]
    ok = {j: bool(check(j, parsed[j])) for j in dense}
    seal = [bool(valid[j]) and ok.get(j, False) for j in range(len(parsed))]
    return seal, sum(1 for j, p in enumerate(parsed) if is_commit(p, rset[j])), len(dense), dense


def views(rows, seal, views_cap, sets, proposers=None):
    """rows as wire_views_model.views takes them, seal: the rows' seal bits → (out_view, stored, n_views, records): the views
    model's answer with every COMMIT record marked and tallied over stored ∧ sealed"""
    view, stored, n_views, records = VM.views(rows, views_cap, sets, proposers)
    out = []
    for v, r in enumerate(records):
        r = dict(r, pad=bytes(5))
        if r["type"] == COMMIT:
            sv = [rows[i][6] for i in range(len(rows)) if view[i] == v and stored[i] and seal[i]]
            r["pad"] = bytes([1, 0, 0, 0, 0])
            r["sealed_senders"] = sv
            r["tally"] = VM.tally(sets[r["set"]], sv)
        out.append(r)
    return view, stored, n_views, out
