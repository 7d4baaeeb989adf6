// host_cert_decide_harness.hip — TEST-ONLY: cert_decide_dev.h (the proposer table, valid_pc / round_change per record, the clauses
// of `proposal`, the selection of the highest prepared round) and the resumed sponge of cert_wave_dev.h on the CPU, so that
// tests/test_dev_cert_decide_host.py can check the exact device source without a GPU.  cdh_decide walks the records the way
// cert_decide_records_kernel / cert_decide_proposals_kernel do, one child after the other instead of a lane each, and closes
// clause (i) with the lane form of the proposal hash; the cross-lane selection and the sponge that starts from a saved state run
// on the 64-coroutine lockstep emulator of wave_emul.h.  Built with hipcc's host pass; never linked into libibftgpu.so, never a
// fallback.
#define IBFT_WAVE_EMUL 1
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "cert_decide_dev.h"
#include "cert_wave_dev.h"

namespace {

alignas(16) uint64_t g_A[32], g_B[32];  // what is LDS on the device

struct select_job {
  const int8_t *valid_pc;
  const uint64_t *pc_round;
  uint32_t n;
  certd::candidate out[64];
  int after[64];
};
void lane_select(void *p) {
  select_job *j = (select_job *)p;
  const uint32_t lane = cw::lane_id();
  certd::candidate best{0ull, 0u, 0u};
  bool undecided = false;
  for (uint32_t k = lane; k < j->n; k += 64u) certd::child_step(best, undecided, j->valid_pc[k], j->pc_round[k], k);
  const certd::candidate win = certd::wave_select(best, lane);
  j->out[lane] = win;
  j->after[lane] = certd::proposal_after_children(cw::ballot(undecided) != 0, win);
}

struct sponge_job {
  const uint8_t *raw;
  uint32_t raw_len;
  uint64_t round;
  uint64_t *mid;  // 25 words
  bool resume;    // false: the whole message, the state behind raw's full blocks → mid; true: from mid
  uint64_t out[4];
};
void lane_sponge(void *p) {
  sponge_job *j = (sponge_job *)p;
  const uint32_t lane = cw::lane_id();
  const uint32_t full = j->raw_len / 136u * 136u;
  const uint64_t tail = keccak::round_tail(j->round);
  const uint64_t w = j->resume ? cw::sponge_message_from(j->raw, j->raw_len, 0u, j->raw_len + 8u, tail, true, lane, g_A, g_B,
                                                         j->mid[cw::sponge_word(lane)], full, nullptr, 0u)
                               : cw::sponge_message_from(j->raw, j->raw_len, 0u, j->raw_len + 8u, tail, true, lane, g_A, g_B, 0ull, 0u, j->mid, full);
  if (lane < 4) j->out[lane] = w;
}
void lane_sponge_plain(void *p) {
  sponge_job *j = (sponge_job *)p;
  const uint32_t lane = cw::lane_id();
  const uint64_t w = cw::sponge_message(j->raw, j->raw_len, 0u, j->raw_len + 8u, keccak::round_tail(j->round), true, lane, g_A, g_B);
  if (lane < 4) j->out[lane] = w;
}

}  // namespace

extern "C" {

uint32_t cdh_decision_size() { return (uint32_t)sizeof(certd::decision); }

int cdh_is_proposer(uint64_t t_height, uint64_t t_first, uint32_t t_rounds, const uint8_t *t_addr20, const uint8_t *who, uint32_t who_len, uint64_t h,
                    uint64_t r) {
  const certd::proposer_table t{t_height, t_first, t_addr20, t_rounds};
  return certd::is_proposer(t, who, who_len, h, r);
}

// One decision per record of `rec` (n_records of them, the first n_roots are the rows 0 … n_roots − 1) under the table; wire: the
// call's bytes (the raw proposals lie there).  → 0, or −1 when a record names rows or records that do not exist.
int cdh_decide(const wire::node_info *nodes, const wire::row_info *rows, const certv::record *rec, uint32_t n_roots, uint32_t n_rows, uint32_t n_records,
               uint64_t t_height, uint64_t t_first, uint32_t t_rounds, const uint8_t *t_addr20, const uint8_t *wire_bytes, certd::decision *out) {
  const certd::proposer_table t{t_height, t_first, t_addr20, t_rounds};
  for (uint32_t i = 0; i < n_records; i++) {
    const certv::record &r = rec[i];
    const bool root = i < n_roots;
    uint64_t height = r.height;
    bool known = true;
    if (!root) {
      const uint32_t parent = r.row < n_rows ? nodes[r.row].parent : wire::NO_PARENT;
      known = parent < n_roots;
      height = known ? rec[parent].height : 0ull;
    }
    certd::decide_record(out[i], r, root, height, known, t);
  }
  for (uint32_t root = 0; root < n_roots; root++) {
    const certv::record &r = rec[root];
    if (r.row != root || root >= n_rows) return -1;
    int v = certd::proposal_head(r, rows[root], nodes[root], true, t);
    if (v != certd::GO) {
      out[root].proposal = (int8_t)v;
      continue;
    }
    const uint32_t first = r.first_child_cert, n = r.n_children;
    if (first == certv::NO_RECORD || first < n_roots || (uint64_t)first + n > n_records) return -1;
    certd::candidate best{0ull, 0u, 0u};
    bool undecided = false;
    for (uint32_t k = 0; k < n; k++) certd::child_step(best, undecided, out[first + k].valid_pc, rec[first + k].pc_round, k);
    v = certd::proposal_after_children(undecided, best);
    if (v != certd::GO) {
      out[root].proposal = (int8_t)v;
      continue;
    }
    const certv::record &w = rec[first + best.k];
    uint64_t h[4];
    wire::hash_proposal(wire_bytes + nodes[root].raw_off, nodes[root].raw_len, w.pc_round, h);
    certd::record_prepared(out[root], first + best.k, w, memcmp(h, w.pc_hash, 32) == 0);
  }
  return 0;
}

// The selection on the emulated wavefront: children k with valid_pc[k] and pc_round[k], lane k mod 64 steps over child k.
// → what proposal_after_children answers (−1, 1, 3 = GO); has / k / round of the winner as EVERY lane holds them (−2: the lanes disagree)
int cdh_select(const int8_t *valid_pc, const uint64_t *pc_round, uint32_t n, uint32_t *has, uint32_t *k, uint64_t *round) {
  select_job j{};
  j.valid_pc = valid_pc, j.pc_round = pc_round, j.n = n;
  wave_emul::run(lane_select, &j);
  for (int l = 1; l < 64; l++)
    if (j.out[l].has != j.out[0].has || j.after[l] != j.after[0] || (j.out[0].has && (j.out[l].k != j.out[0].k || j.out[l].round != j.out[0].round))) return -2;
  *has = j.out[0].has, *k = j.out[0].k, *round = j.out[0].round;
  return j.after[0];
}

// keccak256(raw ‖ BE64(round0)) by the whole sponge, which leaves its state behind raw's full blocks in mid25; then
// keccak256(raw ‖ BE64(round1)) from that state.  raw must carry 16 bytes of slack.
void cdh_resumed_proposal_hash(const uint8_t *raw, uint32_t raw_len, uint64_t round0, uint64_t round1, uint64_t *mid25, uint8_t *out32_whole,
                               uint8_t *out32_resumed) {
  sponge_job j{raw, raw_len, round0, mid25, false, {0, 0, 0, 0}};
  wave_emul::run(lane_sponge, &j);
  memcpy(out32_whole, j.out, 32);
  sponge_job r{raw, raw_len, round1, mid25, true, {0, 0, 0, 0}};
  wave_emul::run(lane_sponge, &r);
  memcpy(out32_resumed, r.out, 32);
}
// cw::sponge_message as every other caller uses it
void cdh_proposal_hash(const uint8_t *raw, uint32_t raw_len, uint64_t round, uint8_t *out32) {
  sponge_job j{raw, raw_len, round, nullptr, false, {0, 0, 0, 0}};
  wave_emul::run(lane_sponge_plain, &j);
  memcpy(out32, j.out, 32);
}

}  // extern "C"
