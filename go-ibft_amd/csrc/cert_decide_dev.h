// cert_decide_dev.h — what is left of the reference's certificate rules once IsProposer can be answered on the device, written
// once for the device and for the CPU (ibft_decide_certificates_wire; kernels.hip.h: cert_decide_records_kernel,
// cert_decide_proposals_kernel; host_cert_decide_harness.hip):
//
//   the proposer table of ONE height (ibft_set_proposers), its lookup and the three-valued IsProposer over it;
//   valid_pc      validPC whole (core/ibft.go:1162-1231): the record's pc (cert_verdict_dev.h) with the proposer rule;
//   round_change  handleRoundChangeMessage's closure (:478-489) for a root ROUND_CHANGE;
//   proposal      validateProposalCommon / validateProposal0 / validateProposal (:640-787) for a root PREPREPARE, clause by
//                 clause in the reference's order: a HEAD over the record's own row (clauses a–f), a STEP per record of its
//                 RoundChangeCertificate, the SELECTION of the highest prepared round across the lanes, and the closing
//                 comparison keccak256(raw ‖ BE64(prepared_round)) == prepared_hash, which the kernel computes from the sponge
//                 state the digest stage left behind the full blocks of raw (cert_wave_dev.h: sponge_message_from).
//
// Values: −1 undecided here, 0 false, 1 true (valid_pc also 2: the message carries no certificate).  Undecided never hides a
// false that precedes it: the clauses are walked in order and the first one that is not true decides.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cert_verdict_dev.h"
#if !defined(__HIP_DEVICE_COMPILE__) && defined(IBFT_WAVE_EMUL)
#include "wave_emul.h"  // tests only
#endif

namespace certd {

constexpr int UNDECIDED = -1, NO = 0, YES = 1;
constexpr int GO = 3;  // a head's answer: the certificate's records decide
constexpr uint32_t PROPOSER_ROUNDS_MAX = 4096;  // IBFT_PROPOSER_ROUNDS_MAX
constexpr uint8_t HAS_PREPARED = 1;             // IBFT_CERT_DECISION_HAS_PREPARED

// mirrors ibft_cert_decision_t (include/ibftgpu.h), 64 bytes
struct decision {
  int8_t valid_pc, round_change, proposal;
  uint8_t flags;
  uint32_t prepared_record;
  uint64_t prepared_round;
  uint8_t prepared_hash[32];
  uint8_t reserved[16];
};
static_assert(sizeof(decision) == 64, "ABI");

// ---- the proposer table ------------------------------------------------------------------------------------------------
// the proposers of rounds [first_round, first_round + n_rounds) of `height`, 20 bytes each; n_rounds == 0: no table
struct proposer_table {
  uint64_t height, first_round;
  const uint8_t *addr20;
  uint32_t n_rounds;
};
// T(h, r): the entry, or null (UNKNOWN) — no table, another height, a round outside the range
HD const uint8_t *table_lookup(const proposer_table &t, uint64_t h, uint64_t r) {
  if (t.n_rounds == 0 || t.n_rounds > PROPOSER_ROUNDS_MAX || h != t.height || r < t.first_round || r - t.first_round >= t.n_rounds) return nullptr;
  return t.addr20 + 20ull * (r - t.first_round);
}
HD int is_proposer(const proposer_table &t, const uint8_t *who, uint32_t who_len, uint64_t h, uint64_t r) {
  const uint8_t *p = table_lookup(t, h, r);
  if (!p) return UNDECIDED;
  if (who_len != 20) return NO;
  bool eq = true;
  for (int i = 0; i < 20; i++) eq = eq && who[i] == p[i];
  return eq ? YES : NO;
}

// ---- per record --------------------------------------------------------------------------------------------------------
// validPC whole.  height: the record's own for a root, the parent PREPREPARE's for a record of its certificate; height_known =
// false (a record whose parent cannot be named) leaves the proposer rule undecided.
HD int valid_pc(const certv::record &r, uint64_t height, bool height_known, const proposer_table &t) {
  if (r.pc != certv::VALID) return r.pc;
  return height_known ? is_proposer(t, r.pc_from, 20, height, r.pc_round) : UNDECIDED;
}
// a root record whose row is a judged ROUND_CHANGE; −1 for every other record
HD int round_change(const certv::record &r, bool root, int vpc) {
  if (!root || (r.cls & 1u) || r.type != certv::TYPE_ROUND_CHANGE) return UNDECIDED;
  if (vpc == certv::NO_CERTIFICATE) return (r.bits & certv::BIT_HAS_PROPOSAL) ? NO : YES;
  return vpc;
}
// everything of a decision but `proposal` of a root PREPREPARE (which stays −1 here)
HD void decide_record(decision &d, const certv::record &r, bool root, uint64_t height, bool height_known, const proposer_table &t) {
  const int vpc = valid_pc(r, height, height_known, t);
  d.valid_pc = (int8_t)vpc;
  d.round_change = (int8_t)round_change(r, root, vpc);
  d.proposal = (int8_t)UNDECIDED;
  d.flags = 0;
  d.prepared_record = certv::NO_RECORD;
  d.prepared_round = 0;
  for (int i = 0; i < 32; i++) d.prepared_hash[i] = 0;
  for (int i = 0; i < 16; i++) d.reserved[i] = 0;
}

// ---- proposal: the head ------------------------------------------------------------------------------------------------
// a regular PREPREPARE: class 0, judged, with a view, type and payload agree
HD bool regular_preprepare(const certv::record &r, const wire::row_info &ri) {
  return r.cls == 0 && ri.status == wire::STATUS_OK && ri.has_view && ri.type == certv::TYPE_PREPREPARE && ri.payload_kind == wire::KIND_PREPREPARE;
}
// clauses (a) … (f) over the root's own record, row and node; GO: rcc == 1, the records of its certificate decide
HD int proposal_head(const certv::record &r, const wire::row_info &ri, const wire::node_info &nd, bool root, const proposer_table &t) {
  if (!root || !regular_preprepare(r, ri)) return UNDECIDED;
  if (!(nd.flags & wire::TREE_HAS_PROPOSAL)) return NO;      // (a) a nil proposal
  if (nd.proposal_round != ri.round) return NO;               // (b)
  const int p = is_proposer(t, ri.from, ri.from_len, ri.height, ri.round);  // (c)
  if (p != YES) return p;
  if (!(r.bits & certv::BIT_SELF)) return NO;                 // (d) IsValidProposalHash(proposal, hash)
  if (ri.round == 0) return YES;                              // (e) validateProposal0 never looks at a certificate
  if (r.rcc == certv::UNDECIDED) return UNDECIDED;            // (f)
  if (r.rcc != certv::VALID) return NO;
  return GO;
}

// ---- proposal: the certificate's records -------------------------------------------------------------------------------
// a lane's best child so far: the pair (pc_round, child index), the larger pair wins — so the LAST among equal rounds does,
// whichever lane saw it
struct candidate {
  uint64_t round;
  uint32_t k;
  uint32_t has;
};
HD bool better(const candidate &a, const candidate &b) {  // a beats b
  if (a.has != b.has) return a.has != 0;
  if (!a.has) return false;
  if (a.round != b.round) return a.round > b.round;
  return a.k > b.k;
}
// child k of the certificate: its valid_pc (cert_decide_records_kernel) and the round of its prepared certificate
HD void child_step(candidate &best, bool &undecided, int child_valid_pc, uint64_t pc_round, uint32_t k) {
  if (child_valid_pc == UNDECIDED) undecided = true;
  if (child_valid_pc != YES) return;
  const candidate c{pc_round, k, 1u};
  if (better(c, best)) best = c;
}

HD uint32_t shfl_xor_u32(uint32_t v, uint32_t mask, uint32_t lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)lane;
  return (uint32_t)__shfl_xor((int)v, (int)mask, 64);
#elif defined(IBFT_WAVE_EMUL)
  return wave_emul::xchg(v, (int)(lane ^ mask), 0x5E1E0000u | mask);
#else
  (void)mask, (void)lane;
  return v;  // one lane: the serial walk of the CPU harness
#endif
}
// the best candidate of the wavefront, in every lane
HD candidate wave_select(candidate c, uint32_t lane) {
  for (uint32_t o = 32; o; o >>= 1) {
    candidate p;
    p.round = (uint64_t)shfl_xor_u32((uint32_t)c.round, o, lane) | ((uint64_t)shfl_xor_u32((uint32_t)(c.round >> 32), o, lane) << 32);
    p.k = shfl_xor_u32(c.k, o, lane);
    p.has = shfl_xor_u32(c.has, o, lane);
    if (better(p, c)) c = p;
  }
  return c;
}
// clauses (g), (h) behind the children; GO: (i) — the winner's hash against the proposal's under the winner's round
HD int proposal_after_children(bool a_child_is_undecided, const candidate &winner) {
  if (a_child_is_undecided) return UNDECIDED;  // (g)
  if (!winner.has) return YES;                  // (h) nobody prepared anything
  return GO;
}
// (i) reached: the winner goes into the decision whether the hashes agree or not
HD void record_prepared(decision &d, uint32_t prepared_record, const certv::record &winner, bool hash_matches) {
  d.flags = HAS_PREPARED;
  d.prepared_record = prepared_record;
  d.prepared_round = winner.pc_round;
  for (int i = 0; i < 32; i++) d.prepared_hash[i] = winner.pc_hash[i];
  d.proposal = (int8_t)(hash_matches ? YES : NO);
}

}  // namespace certd
