// host_round_change_harness.hip — TEST-ONLY: the row and record bodies of the round_change_*_kernel launches (round_change_dev.h
// over wire_views_dev.h's tables) on the CPU, so that tests/test_dev_round_change_host.py can check the exact device source
// without a GPU: the participation rule, the two tables filled in any row order, representatives and ranks, out_rc_view /
// out_rc_stored, the per-key sums, rcd::key_record and the answer.  The cross-row parts — the scan of the representatives, the
// sums — are plain loops here where the kernels have their workgroup scan and their wavefront turns; the answer's selection runs
// serially in rch_run and on the 64-coroutine lockstep emulator of wave_emul.h in rch_select.  Built with hipcc's host pass;
// never linked into libibftgpu.so, never a fallback.
#define IBFT_WAVE_EMUL 1
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "round_change_dev.h"

namespace {

struct select_job {
  const rcd::record *recs;
  uint32_t filled, n_keys, cap, unjudged;
  rcd::query q;
  rcd::answer out[64];
};
void lane_select(void *p) {
  select_job *j = (select_job *)p;
  const uint32_t lane = (uint32_t)wave_emul::lane();
  rcd::lane_state s = rcd::lane_init();
  for (uint32_t i = lane; i < j->filled; i += 64u) rcd::record_step(s, j->recs[i], i, j->q);
  const rcd::lane_state w = rcd::wave_state(s, lane);
  rcd::make_answer(j->out[lane], w, j->n_keys, j->cap, j->unjudged);
}

}  // namespace

extern "C" {

uint32_t rch_sizeof(int which) {
  return (uint32_t)(which == 0 ? sizeof(rcd::query) : which == 1 ? sizeof(rcd::record) : sizeof(rcd::answer));
}

// the validator table as ibft_set_validators builds it: slots × 6 words {addr[5], index + 1}; → the slot mask
uint32_t rch_build_vtab(const uint8_t *addrs20, uint32_t n_validators, uint32_t *tab, uint32_t slots) {
  for (uint32_t i = 0; i < 6 * slots; i++) tab[i] = 0;
  for (uint32_t u = 0; u < n_validators; u++) {
    uint32_t a[5];
    memcpy(a, addrs20 + 20ull * u, 20);
    uint32_t s = ibftk::addr_hash(a) & (slots - 1);
    while (tab[6 * s + 5]) s = (s + 1) & (slots - 1);
    memcpy(tab + 6 * s, a, 20);
    tab[6 * s + 5] = u + 1;
  }
  return slots - 1;
}

// The whole stage over the n level-0 rows (80 bytes each) with their records (128) and decisions (64); rows are INSERTED in
// the order `order` names.  tables: 2 × slots words, left as filled.  query may be null (no answer).  → 0, or 1 when a table
// was exhausted (then only the tables are meaningful).
int rch_run(const uint8_t *rows80, const uint8_t *rec128, const uint8_t *dec64, uint32_t n, const uint32_t *order, uint32_t slots, uint32_t salt,
            uint32_t rc_cap, const uint32_t *vtab, uint32_t vslot_mask, uint32_t n_validators, const uint32_t *vpower32, uint32_t n_pieces,
            const uint64_t *quorum, const uint8_t *query32, uint32_t *tables, int32_t *out_view, uint64_t *out_stored, uint8_t *out_rc,
            uint32_t *out_n_rc, uint8_t *out_answer) {
  const wire::row_info *rows = reinterpret_cast<const wire::row_info *>(rows80);
  const certv::record *rec = reinterpret_cast<const certv::record *>(rec128);
  const certd::decision *dec = reinterpret_cast<const certd::decision *>(dec64);
  std::vector<int32_t> vidx(n, -1);
  uint32_t unjudged = 0;
  // the index launch: every row's entry, before the first insert (insert_row compares the entries of other rows)
  for (uint32_t r = 0; r < n; r++) vidx[r] = rcd::row_index(rec[r], rows[r], vtab, vslot_mask, n_validators);
  for (uint32_t r = 0; r < n; r++)
    if (rcd::unjudged(rec[r])) unjudged++;
  const wviews::columns k{rows, vidx.data()};
  uint32_t *key_table = tables, *last_table = tables + slots;
  for (uint32_t i = 0; i < 2 * slots; i++) tables[i] = wviews::EMPTY;
  std::vector<wviews::row_slots> sl(n);
  int err = 0;
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t r = order[j];
    sl[r] = wviews::insert_row(k, r, vidx[r] >= 0, key_table, last_table, slots, salt);
    if (sl[r].key == wviews::UNPLACED || sl[r].last == wviews::UNPLACED) err = 1;
  }
  if (err) return 1;
  std::vector<uint32_t> rank_of(n, 0), first_row;
  for (uint32_t r = 0; r < n; r++)
    if (wviews::is_rep(key_table, sl[r].key, r)) {
      rank_of[r] = (uint32_t)first_row.size();
      first_row.push_back(r);
    }
  const uint32_t n_keys = (uint32_t)first_row.size(), cap = rc_cap < n ? rc_cap : n;
  *out_n_rc = n_keys;
  const uint32_t words = (uint32_t)rcd::acc_words((int)n_pieces);
  std::vector<uint64_t> acc((size_t)cap * words + 1, 0);
  for (uint32_t w = 0; w < (n + 63) / 64; w++) out_stored[w] = 0;
  for (uint32_t r = 0; r < n; r++) {
    out_view[r] = rcd::VIEW_NONE;
    if (sl[r].key >= wviews::SKIP) continue;
    const int32_t v = wviews::view_of_rank(rank_of[key_table[sl[r].key]], cap);
    const bool stored = wviews::is_stored(last_table, sl[r].last, r);
    out_view[r] = v;
    if (stored) out_stored[r >> 6] |= 1ull << (r & 63);
    if (v < 0) continue;
    uint64_t *a = &acc[(size_t)v * words];
    a[2 * n_pieces] += 1ull | ((uint64_t)(stored ? 1u : 0u) << 32);
    const int rc = stored ? (int)dec[r].round_change : 0;
    if (rc == certd::YES || rc == certd::UNDECIDED) {
      const uint32_t at = rc == certd::YES ? 0u : n_pieces;
      for (uint32_t i = 0; i < n_pieces; i++) a[at + i] += vpower32[(size_t)vidx[r] * n_pieces + i];
      a[2 * n_pieces + 1] += rc == certd::YES ? 1ull : 1ull << 32;
    }
  }
  std::vector<rcd::record> recs(cap ? cap : 1);
  for (uint32_t v = 0; v < cap; v++) {
    if (v < n_keys) rcd::key_record(recs[v], first_row[v], rows[first_row[v]], &acc[(size_t)v * words], (int)n_pieces, quorum);
    else rcd::empty_record(recs[v]);
  }
  memcpy(out_rc, recs.data(), (size_t)cap * sizeof(rcd::record));
  if (query32) {
    rcd::query q;
    memcpy(&q, query32, sizeof q);
    rcd::lane_state s = rcd::lane_init();
    for (uint32_t i = 0; i < n_keys && i < cap; i++) rcd::record_step(s, recs[i], i, q);
    rcd::answer ans;
    rcd::make_answer(ans, s, n_keys, cap, unjudged);
    memcpy(out_answer, &ans, sizeof ans);
  }
  return 0;
}

// The selection on the emulated wavefront over `filled` records, lane l striding over records l, l + 64, …  → 0 and the answer
// as EVERY lane computes it, or −2 when the lanes disagree.
int rch_select(const uint8_t *recs128, uint32_t filled, uint32_t n_keys, uint32_t cap, uint32_t unjudged, const uint8_t *query32, uint8_t *out_answer) {
  select_job j{};
  j.recs = reinterpret_cast<const rcd::record *>(recs128);
  j.filled = filled, j.n_keys = n_keys, j.cap = cap, j.unjudged = unjudged;
  memcpy(&j.q, query32, sizeof j.q);
  wave_emul::run(lane_select, &j);
  for (int l = 1; l < 64; l++)
    if (memcmp(&j.out[l], &j.out[0], sizeof(rcd::answer)) != 0) return -2;
  memcpy(out_answer, &j.out[0], sizeof(rcd::answer));
  return 0;
}

}  // extern "C"
