// cert_verdict_dev.h — the certificate rules of the reference over the rows of a certificate tree, written once for the device
// and for the CPU (ibft_judge_certificates_wire; kernels.hip.h: cert_judge_kernel; host_cert_verdict_harness.hip):
//
//   pc   validPC (core/ibft.go:1162-1231) with AreValidPCMessages / HasUniqueSenders (messages/helpers.go:148-213) and, with
//        match_proposal, proposalMatchesCertificate (core/ibft.go:516-551), for the PreparedCertificate of a ROUND_CHANGE row —
//        everything but IsProposer, which is the Backend's;
//   rcc  the RoundChangeCertificate half of validateProposal (core/ibft.go:697-778) for a PREPREPARE row.
//
// Values: −1 undecided here (an irregular shape: the walk over the decoded objects is the authority), 0 invalid, 1 valid
// (pc: up to the proposer rule), 2 the message carries no certificate.  The two functions are HotPath::pcVerdictFromRows and
// HotPath::proposalVerdictFromRows (host/backend.cpp) taken apart: a HEAD over the carrier's own row, a STEP per child that
// returns a flag word, and a FOLD of the OR of those flags with "every child a distinct validator" and "their power reaches
// the quorum".  The fold keeps the order in which the host functions' return statements occur: F_UNDECIDED (−1) before
// F_WRONG_TYPE (0) before F_WRONG_KIND (−1) before everything else (0).
//
// Why distinct validators and power may be counted over the rows whose sender bit is set, by validator index: every −1 of the
// host functions precedes their sender and power clauses, and after those clauses the verdict is a pure AND.  A certificate
// with a sender bit 0 is 0 whatever its power; with every sender bit 1 every From is a 20-byte member of the set, so
// uniqueness by validator index is uniqueness by bytes and the summed power is the host's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wire_dev.h"

namespace certv {

constexpr uint8_t TYPE_PREPREPARE = 0, TYPE_PREPARE = 1, TYPE_ROUND_CHANGE = 3;  // IbftMessage.type
constexpr int UNDECIDED = -1, INVALID = 0, VALID = 1, NO_CERTIFICATE = 2;
constexpr int GO = 3;  // a head's answer: the children decide

constexpr uint32_t F_UNDECIDED = 1;    // a child of an irregular shape: −1
constexpr uint32_t F_WRONG_TYPE = 2;   // pc: the proposal message is no PREPREPARE / another one is no PREPARE: 0
constexpr uint32_t F_WRONG_KIND = 4;   // pc: type and payload disagree, or the hash is not 32 bytes: −1
constexpr uint32_t F_MISMATCH = 8;     // another view (pc: or round ≥ limit, or another hash; rcc: or no ROUND_CHANGE): 0
constexpr uint32_t F_BAD_SENDER = 16;  // IsValidValidator false: 0
constexpr uint32_t F_BAD_HASH = 32;    // pc with match_proposal: IsValidProposalHash false: 0

// mirrors ibft_cert_verdict_t (include/ibftgpu.h), 128 bytes
constexpr uint32_t NO_RECORD = 0xFFFFFFFFu;
constexpr uint8_t BIT_SENDER = 1, BIT_HASH = 2, BIT_SELF = 4, BIT_HAS_PROPOSAL = 8, BIT_HAS_CERTIFICATE = 16;
struct record {
  uint32_t row, first_child, n_children;
  uint32_t first_child_cert;
  uint32_t rcc_rows;
  int8_t pc, rcc;
  uint8_t cls, bits;
  uint8_t type, role, level, from_len;
  uint32_t reserved;
  uint64_t height, round;
  uint64_t pc_round;
  uint8_t from[20];
  uint8_t pc_from[20];
  uint8_t pc_hash[32];
};
static_assert(sizeof(record) == 128, "ABI");

// ---- pc ----------------------------------------------------------------------------------------------------------------
struct pc_params {
  uint64_t height, limit;   // the view the certificate must be of, the round it must lie below
  uint64_t ref_round;       // the round of the certificate's proposal message (its first child)
  const uint8_t *ref_hash;  // the 32 bytes that message carries
  bool match_proposal;
};

// the carrier's own row; GO: the children [first_child, first_child + n_children) decide, there are at least two of them
HD int pc_head(const wire::node_info *nodes, const wire::row_info *rows, const uint8_t *cls, uint32_t n_rows, uint32_t row,
               bool match_proposal) {
  if (row >= n_rows || cls[row] != 0) return UNDECIDED;
  const wire::row_info &rc = rows[row];
  const wire::node_info &nd = nodes[row];
  if (rc.status != wire::STATUS_OK || !rc.has_view || rc.type != TYPE_ROUND_CHANGE || rc.payload_kind != wire::KIND_ROUND_CHANGE)
    return UNDECIDED;
  if (!(nd.flags & wire::TREE_HAS_CERT)) return NO_CERTIFICATE;
  if (match_proposal && !(nd.flags & wire::TREE_HAS_PROPOSAL)) return UNDECIDED;  // IsValidProposalHash(nil, hash): the backend's
  if (nd.n_children == 0) return INVALID;  // no proposal message — before the bounds: a leaf's first_child means nothing
  if ((uint64_t)nd.first_child + nd.n_children > n_rows) return UNDECIDED;
  if (nodes[nd.first_child].role != wire::ROLE_PC_PROPOSAL) return INVALID;  // ProposalMessage == nil
  if (nd.n_children == 1) return INVALID;                                    // PrepareMessages == nil
  return GO;
}

// one child; first: it is the certificate's proposal message
HD uint32_t pc_child(const wire::row_info &w, const wire::node_info &nd, uint8_t cls, bool sender_bit, bool hash_bit, bool first,
                     const pc_params &p) {
  uint32_t f = 0;
  if (cls != 0 || w.status != wire::STATUS_OK || !w.has_view || w.from_len > 20 || nd.n_children != 0 ||
      (!first && nd.role != wire::ROLE_PC_PREPARE))
    f |= F_UNDECIDED;
  if (w.type != (first ? TYPE_PREPREPARE : TYPE_PREPARE)) f |= F_WRONG_TYPE;
  if (w.payload_kind != (first ? wire::KIND_PREPREPARE : wire::KIND_PREPARE) || w.hash_len != 32) f |= F_WRONG_KIND;
  bool same = w.height == p.height && w.round == p.ref_round && w.round < p.limit;
  for (int i = 0; i < 32; i++) same = same && w.proposal_hash[i] == p.ref_hash[i];
  if (!same) f |= F_MISMATCH;
  if (!sender_bit) f |= F_BAD_SENDER;
  if (p.match_proposal && !hash_bit) f |= F_BAD_HASH;
  return f;
}

// flags: the OR over all children; all_distinct: every child's sender bit is set and their validator indices differ
HD int pc_fold(uint32_t flags, bool all_distinct, bool power_reaches_quorum) {
  if (flags & F_UNDECIDED) return UNDECIDED;
  if (flags & F_WRONG_TYPE) return INVALID;
  if (flags & F_WRONG_KIND) return UNDECIDED;
  if ((flags & (F_MISMATCH | F_BAD_SENDER | F_BAD_HASH)) || !all_distinct || !power_reaches_quorum) return INVALID;
  return VALID;
}

// ---- rcc ---------------------------------------------------------------------------------------------------------------
// the PREPREPARE's own row; GO: the children decide (there may be none: the fold answers that)
HD int rcc_head(const wire::node_info *nodes, const wire::row_info *rows, const uint8_t *cls, uint32_t n_rows, uint32_t row) {
  if (row >= n_rows || cls[row] != 0) return UNDECIDED;
  const wire::row_info &pp = rows[row];
  const wire::node_info &nd = nodes[row];
  if (pp.status != wire::STATUS_OK || !pp.has_view || pp.type != TYPE_PREPREPARE || pp.payload_kind != wire::KIND_PREPREPARE)
    return UNDECIDED;
  if (!(nd.flags & wire::TREE_HAS_CERT)) return NO_CERTIFICATE;
  if (nd.n_children && (uint64_t)nd.first_child + nd.n_children > n_rows) return UNDECIDED;
  return GO;
}

// one message of the RoundChangeCertificate of a PREPREPARE of (height, round)
HD uint32_t rcc_child(const wire::row_info &w, const wire::node_info &nd, uint8_t cls, bool sender_bit, uint64_t height, uint64_t round) {
  uint32_t f = 0;
  if (cls != 0 || w.status != wire::STATUS_OK || !w.has_view || w.from_len > 20 || nd.role != wire::ROLE_RCC_MESSAGE) f |= F_UNDECIDED;
  if (w.type == TYPE_ROUND_CHANGE && w.payload_kind != wire::KIND_ROUND_CHANGE) f |= F_UNDECIDED;  // ExtractLatestPC's type / payload rule
  if (w.type != TYPE_ROUND_CHANGE || w.height != height || w.round != round) f |= F_MISMATCH;
  if (!sender_bit) f |= F_BAD_SENDER;
  return f;
}

// the certificate's own clauses; VALID still depends on the children's prepared certificates (rcc_with_children)
HD int rcc_fold(uint32_t flags, uint32_t n_children, bool all_distinct, bool power_reaches_quorum) {
  if (flags & F_UNDECIDED) return UNDECIDED;
  if (n_children == 0) return INVALID;  // HasUniqueSenders of nothing
  if ((flags & (F_MISMATCH | F_BAD_SENDER)) || !all_distinct || !power_reaches_quorum) return INVALID;
  return VALID;
}
// a ROUND_CHANGE message whose prepared certificate is undecided leaves the highest prepared round undecided
HD int rcc_with_children(int rcc, bool a_child_pc_is_undecided) { return rcc == VALID && a_child_pc_is_undecided ? UNDECIDED : rcc; }

// ---- the record's own part ---------------------------------------------------------------------------------------------
HD void record_head(record &r, uint32_t row, const wire::node_info &nd, const wire::row_info &ri, uint8_t cls, bool sender_bit,
                    bool hash_bit, bool self_bit) {
  r.row = row;
  r.first_child = nd.first_child;
  r.n_children = nd.n_children;
  r.first_child_cert = NO_RECORD;
  r.rcc_rows = 0;
  r.pc = r.rcc = (int8_t)UNDECIDED;
  r.cls = cls;
  r.bits = (uint8_t)((sender_bit ? BIT_SENDER : 0) | (hash_bit ? BIT_HASH : 0) | (self_bit ? BIT_SELF : 0) |
                     ((nd.flags & wire::TREE_HAS_PROPOSAL) ? BIT_HAS_PROPOSAL : 0) | ((nd.flags & wire::TREE_HAS_CERT) ? BIT_HAS_CERTIFICATE : 0));
  r.type = ri.type;
  r.role = nd.role;
  r.level = nd.level;
  r.from_len = ri.from_len;
  r.reserved = 0;
  r.height = ri.height;
  r.round = ri.round;
  r.pc_round = 0;
  for (int i = 0; i < 20; i++) r.from[i] = ri.from[i];
  for (int i = 0; i < 20; i++) r.pc_from[i] = 0;
  for (int i = 0; i < 32; i++) r.pc_hash[i] = 0;
}
// pc == VALID: what the caller needs of the certificate's proposal message (IsProposer; the highest prepared round and its hash)
HD void record_pc_proposal(record &r, const wire::row_info &first) {
  r.pc_round = first.round;
  for (int i = 0; i < 20; i++) r.pc_from[i] = first.from[i];
  for (int i = 0; i < 32; i++) r.pc_hash[i] = first.proposal_hash[i];
}

}  // namespace certv
