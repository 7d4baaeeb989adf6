// round_change_dev.h — what handleRoundChangeMessage does with the per-message answers of the decide call
// (ibft_decide_round_changes_wire; core/ibft.go:470-512, messages/messages.go:202-245), written once for the device and for the
// CPU (kernels.hip.h: round_change_*_kernel; host_round_change_harness.hip):
//
//   takes_part    the level-0 row is the ROUND_CHANGE message IBFT.AddMessage would have stored: judged (class 0, status OK,
//                 with a view), type and payload ROUND_CHANGE, a 20-byte From, its sender bit set;
//   sender_index  its From in the validator table (valset_lookup, as cert_judge_kernel finds it); row_index: the column of those
//                 indices, written by a launch of its own IN FRONT of the inserts (insert_row reads other rows' entries);
//   the tables    are wire_views_dev.h's: a ROUND_CHANGE row carries no hash (hash_len 0), so its wviews key is its view
//                 (height, round, type) and its last-table key (view, sender index) — insert_row, is_rep, is_stored as they are;
//   key_record    a key's sums → its record: the tally of the stored rows whose round_change is 1 through tally_record, the
//                 power of the stored rows whose round_change is −1, and the three-valued quorum;
//   the answer    GetExtendedRCC / GetMostRoundChangeMessages over the records: a per-lane pick, a `better` relation and a wave
//                 reduction in the manner of certd::wave_select.
//
// Nothing here depends on the order rows or records are visited in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cert_decide_dev.h"
#include "recover_dev.h"
#include "tally_dev.h"
#include "wire_views_dev.h"

namespace rcd {

constexpr int32_t VIEW_NONE = wviews::VIEW_NONE, VIEW_OVER = wviews::VIEW_OVER;
constexpr uint32_t NO_RECORD = certv::NO_RECORD;
constexpr uint32_t FLAG_OVER = 1;  // IBFT_RC_OVER

// mirror ibft_rc_query_t, ibft_rc_record_t and ibft_rc_answer_t (include/ibftgpu.h)
struct query {
  uint64_t height, round, min_round;
  uint32_t has_accepted_proposal, reserved;
};
struct record {
  uint64_t height, round;
  uint32_t first_row, rows, stored_rows, yes_rows, open_rows;
  int8_t has_quorum;
  uint8_t pad[3];
  uint64_t open_power_lo, open_power_hi;
  wviews::tally_t tally;
  uint8_t reserved[16];
};
struct answer {
  int8_t extended;
  uint8_t pad[3];
  uint32_t flags;
  uint32_t record, most_record;
  uint64_t round, most_round;
  uint32_t most_rows, records_of_height, unjudged_rows;
  uint8_t reserved[20];
};
static_assert(sizeof(query) == 32 && sizeof(record) == 128 && sizeof(answer) == 64, "ABI");

// ---- per row -----------------------------------------------------------------------------------------------------------
HD bool takes_part(const certv::record &r, const wire::row_info &ri) {
  return r.cls == 0 && ri.status == wire::STATUS_OK && ri.has_view && ri.type == certv::TYPE_ROUND_CHANGE &&
         ri.payload_kind == wire::KIND_ROUND_CHANGE && ri.from_len == 20 && (r.bits & certv::BIT_SENDER);
}
// a level-0 row the tree left to the host
HD bool unjudged(const certv::record &r) { return r.cls != 0; }
HD int sender_index(const wire::row_info &ri, const uint32_t *vtab, uint32_t vslot_mask) {
  uint32_t a[5];
  for (int i = 0; i < 5; i++)
    a[i] = (uint32_t)ri.from[4 * i] | ((uint32_t)ri.from[4 * i + 1] << 8) | ((uint32_t)ri.from[4 * i + 2] << 16) | ((uint32_t)ri.from[4 * i + 3] << 24);
  return ibftk::valset_lookup(vtab, vslot_mask, a);
}
// the index column the tables are keyed by: the sender's validator index of a row that takes part, −1 for every other row
HD int32_t row_index(const certv::record &r, const wire::row_info &ri, const uint32_t *vtab, uint32_t vslot_mask, uint32_t n_validators) {
  if (!takes_part(r, ri)) return -1;
  const int vi = sender_index(ri, vtab, vslot_mask);
  return (uint32_t)vi < n_validators ? (int32_t)vi : -1;  // (a set sender bit names a member)
}

// ---- per key -----------------------------------------------------------------------------------------------------------
// A key's accumulators, acc_words(n_pieces) u64 words: the pieces of the powers of its stored rows with round_change 1, those
// of its stored rows with round_change −1, rows | stored << 32, yes | open << 32.
HD int acc_words(int n_pieces) { return 2 * n_pieces + 2; }

// 1 when the yes rows reach the quorum; 0 when yes and open together stay below it; −1 otherwise
HD int quorum3(bool yes_has_quorum, const uint64_t *yes_piece, const uint64_t *open_piece, int n_pieces, const uint64_t *quorum) {
  if (yes_has_quorum) return certd::YES;
  uint64_t both[ibftk::TALLY_MAX_PIECES], w[ibftk::TALLY_SUM_WORDS];
  for (int i = 0; i < ibftk::TALLY_MAX_PIECES; i++) both[i] = i < n_pieces ? yes_piece[i] + open_piece[i] : 0ull;  // (< 2^53 each)
  ibftk::pieces_to_words(both, n_pieces, w);
  return ibftk::words_ge(w, quorum) ? certd::UNDECIDED : certd::NO;
}

HD void key_record(record &o, uint32_t first_row, const wire::row_info &me, const uint64_t *acc, int n_pieces, const uint64_t *quorum) {
  uint64_t yes[ibftk::TALLY_MAX_PIECES], open[ibftk::TALLY_MAX_PIECES];
  for (int i = 0; i < ibftk::TALLY_MAX_PIECES; i++) {
    yes[i] = i < n_pieces ? acc[i] : 0ull;
    open[i] = i < n_pieces ? acc[n_pieces + i] : 0ull;
  }
  const uint64_t c0 = acc[2 * n_pieces], c1 = acc[2 * n_pieces + 1];
  o.height = me.height;
  o.round = me.round;
  o.first_row = first_row;
  o.rows = (uint32_t)c0;
  o.stored_rows = (uint32_t)(c0 >> 32);
  o.yes_rows = (uint32_t)c1;
  o.open_rows = (uint32_t)(c1 >> 32);
  for (int i = 0; i < 3; i++) o.pad[i] = 0;
  for (int i = 0; i < 16; i++) o.reserved[i] = 0;
  // a key holds at most one stored row per validator: every yes row is a distinct member
  uint64_t rec[4], ow[ibftk::TALLY_SUM_WORDS];
  ibftk::tally_record(yes, n_pieces, (uint64_t)o.yes_rows | ((uint64_t)o.yes_rows << 32), quorum, 0ull, rec);
  ibftk::pieces_to_words(open, n_pieces, ow);
  o.open_power_lo = ow[0];
  o.open_power_hi = ow[1];
  o.tally.quorum_lo = quorum[0];
  o.tally.quorum_hi = quorum[1];
  o.tally.power_lo = rec[0];
  o.tally.power_hi = rec[1];
  o.tally.valid_rows = o.yes_rows;
  o.tally.distinct_senders = o.yes_rows;
  o.tally.has_quorum = (uint32_t)rec[3];
  o.tally.shard_overlap = 0;
  o.tally.proposer_rows = 0;
  o.tally.reserved = 0;
  o.has_quorum = (int8_t)quorum3(rec[3] != 0, yes, open, n_pieces, quorum);
}
HD void empty_record(record &o) {
  uint8_t *p = reinterpret_cast<uint8_t *>(&o);
  for (uint32_t i = 0; i < sizeof(record); i++) p[i] = 0;
}

// ---- the answer --------------------------------------------------------------------------------------------------------
// a pick among records: the larger `major` wins, among equals the smaller `minor`, among equals the lower record
struct pick {
  uint64_t major, minor;
  uint32_t rec, has;
};
HD bool better(const pick &a, const pick &b) {  // a beats b
  if (a.has != b.has) return a.has != 0;
  if (!a.has) return false;
  if (a.major != b.major) return a.major > b.major;
  if (a.minor != b.minor) return a.minor < b.minor;
  return a.rec < b.rec;
}
// what a lane has seen of the records it strode over
struct lane_state {
  pick quorum, open, most;  // highest round with has_quorum 1, with has_quorum −1; most stored rows, lowest round among equals
  uint32_t of_height;
};
HD lane_state lane_init() {
  const pick none{0ull, 0ull, NO_RECORD, 0u};
  return lane_state{none, none, none, 0u};
}
HD void record_step(lane_state &s, const record &r, uint32_t index, const query &q) {
  if (r.height != q.height) return;
  s.of_height++;
  if (r.round >= 1 && !(q.has_accepted_proposal && r.round == q.round)) {  // GetExtendedRCC: highestRound starts at 0
    const pick c{r.round, 0ull, index, 1u};
    if (r.has_quorum == certd::YES && better(c, s.quorum)) s.quorum = c;
    if (r.has_quorum == certd::UNDECIDED && better(c, s.open)) s.open = c;
  }
  if (r.round >= 1 && r.round >= q.min_round) {  // GetMostRoundChangeMessages
    const pick c{r.stored_rows, r.round, index, 1u};
    if (better(c, s.most)) s.most = c;
  }
}
HD uint64_t shfl_xor_u64(uint64_t v, uint32_t mask, uint32_t lane) {
  return (uint64_t)certd::shfl_xor_u32((uint32_t)v, mask, lane) | ((uint64_t)certd::shfl_xor_u32((uint32_t)(v >> 32), mask, lane) << 32);
}
// the best pick of the wavefront, in every lane
HD pick wave_pick(pick c, uint32_t lane) {
  for (uint32_t o = 32; o; o >>= 1) {
    pick p;
    p.major = shfl_xor_u64(c.major, o, lane);
    p.minor = shfl_xor_u64(c.minor, o, lane);
    p.rec = certd::shfl_xor_u32(c.rec, o, lane);
    p.has = certd::shfl_xor_u32(c.has, o, lane);
    if (better(p, c)) c = p;
  }
  return c;
}
HD uint32_t wave_add_u32(uint32_t v, uint32_t lane) {
#if defined(__HIP_DEVICE_COMPILE__) || defined(IBFT_WAVE_EMUL)
  for (uint32_t o = 32; o; o >>= 1) v += certd::shfl_xor_u32(v, o, lane);
#else
  (void)lane;  // one lane: the serial walk of the CPU harness
#endif
  return v;
}
// the wavefront's state, in every lane
HD lane_state wave_state(const lane_state &s, uint32_t lane) {
  lane_state w;
  w.quorum = wave_pick(s.quorum, lane);
  w.open = wave_pick(s.open, lane);
  w.most = wave_pick(s.most, lane);
  w.of_height = wave_add_u32(s.of_height, lane);
  return w;
}
HD void make_answer(answer &a, const lane_state &w, uint32_t n_keys, uint32_t cap, uint32_t unjudged_rows) {
  uint8_t *p = reinterpret_cast<uint8_t *>(&a);
  for (uint32_t i = 0; i < sizeof(answer); i++) p[i] = 0;
  const bool open_above = w.open.has && (!w.quorum.has || w.open.major > w.quorum.major);
  a.extended = (int8_t)(open_above ? certd::UNDECIDED : w.quorum.has ? certd::YES : certd::NO);
  a.flags = n_keys > cap ? FLAG_OVER : 0u;
  a.record = w.quorum.has ? w.quorum.rec : NO_RECORD;
  a.round = w.quorum.has ? w.quorum.major : 0ull;
  a.most_record = w.most.has ? w.most.rec : NO_RECORD;
  a.most_round = w.most.has ? w.most.minor : 0ull;
  a.most_rows = w.most.has ? (uint32_t)w.most.major : 0u;
  a.records_of_height = w.of_height;
  a.unjudged_rows = unjudged_rows;
}

}  // namespace rcd
