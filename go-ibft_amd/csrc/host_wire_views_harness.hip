// host_wire_views_harness.hip — TEST-ONLY: the row bodies of the wire_views_*_kernel launches (wire_views_dev.h) on the CPU, so
// that tests/test_dev_wire_views_host.py can check the exact device source without a GPU: the two tables filled in any row
// order, representatives and ranks, out_view / out_stored, the per-view sums and wviews::view_record.  The cross-row parts —
// the scan of the representatives, the sums — are plain loops here where the kernels have their workgroup scan and their
// wavefront turns.  Built with hipcc's host pass; never linked into libibftgpu.so, never a fallback.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "wire_views_dev.h"

extern "C" {

uint32_t wvh_table_slots(uint32_t n, uint32_t hook) { return wviews::table_slots(n, hook); }
uint32_t wvh_sizeof_view(void) { return (uint32_t)sizeof(wviews::view_t); }

// where row `row` starts probing in the key table / the last table (tests measure the probe runs of their inputs)
void wvh_hashes(const uint8_t *rows80, const int32_t *vidx, uint32_t n, uint32_t salt, uint32_t *out_key, uint32_t *out_last) {
  const wire::row_info *rows = reinterpret_cast<const wire::row_info *>(rows80);
  for (uint32_t i = 0; i < n; i++) {
    out_key[i] = wviews::key_hash(rows[i], salt);
    out_last[i] = wviews::last_hash(rows[i], vidx[i], salt);
  }
}

struct wvh_family {
  const int32_t *setidx;
  const uint32_t *set_meta, *vpower32;
  const uint64_t *quorum;
  const uint32_t *vtab;
  uint32_t vslot_mask, n_union, n_pieces;
  // the proposer table
  uint64_t t_height, t_first;
  const uint8_t *t_addr20;
  uint32_t t_rounds;
};

// The whole stage over n parsed rows (80 bytes each), valid[i] = the final verdict bit, vidx / row_set as the sets tally left
// them; rows are INSERTED in the order `order` names (n row numbers).  Tables: 2 × slots words, left as filled.  → 0, or 1
// when a table was exhausted (then only the tables and the slots are meaningful).
int wvh_run(const uint8_t *rows80, const int32_t *vidx, const int32_t *row_set, const uint8_t *valid, uint32_t n, const uint32_t *order,
            uint32_t slots, uint32_t salt, uint32_t views_cap, const wvh_family *fam, uint32_t *tables, int32_t *out_view, uint64_t *out_stored,
            uint8_t *out_views, uint32_t *out_n_views) {
  const wire::row_info *rows = reinterpret_cast<const wire::row_info *>(rows80);
  const wviews::columns k{rows, vidx};
  uint32_t *key_table = tables, *last_table = tables + slots;
  for (uint32_t i = 0; i < 2 * slots; i++) tables[i] = wviews::EMPTY;
  std::vector<wviews::row_slots> sl(n);
  int err = 0;
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t r = order[j];
    sl[r] = wviews::insert_row(k, r, valid[r] != 0, key_table, last_table, slots, salt);
    if (sl[r].key == wviews::UNPLACED || sl[r].last == wviews::UNPLACED) err = 1;
  }
  if (err) return 1;
  // ranks of the representatives in ascending row order
  std::vector<uint32_t> rank_of(n, 0), first_row;
  for (uint32_t r = 0; r < n; r++)
    if (wviews::is_rep(key_table, sl[r].key, r)) {
      rank_of[r] = (uint32_t)first_row.size();
      first_row.push_back(r);
    }
  const uint32_t n_views = (uint32_t)first_row.size();
  *out_n_views = n_views;
  const uint32_t np = fam->n_pieces, cap = views_cap < n ? views_cap : n;
  std::vector<uint64_t> acc((size_t)cap * (np + 1) + 1, 0);
  for (uint32_t w = 0; w < (n + 63) / 64; w++) out_stored[w] = 0;
  for (uint32_t r = 0; r < n; r++) {
    out_view[r] = wviews::VIEW_NONE;
    if (sl[r].key >= wviews::SKIP) continue;
    const int32_t v = wviews::view_of_rank(rank_of[key_table[sl[r].key]], cap);
    const bool stored = wviews::is_stored(last_table, sl[r].last, r);
    out_view[r] = v;
    if (stored) out_stored[r >> 6] |= 1ull << (r & 63);
    if (v < 0) continue;
    uint64_t *a = &acc[(size_t)v * (np + 1)];
    a[np] += 1ull | ((uint64_t)(stored ? 1u : 0u) << 32);
    if (stored) {
      const uint32_t entry = reinterpret_cast<const uint2 *>(fam->set_meta)[row_set[r]].x + (uint32_t)vidx[r];
      for (uint32_t i = 0; i < np; i++) a[i] += fam->vpower32[(size_t)entry * np + i];
    }
  }
  wviews::family f;
  f.setidx = fam->setidx;
  f.set_meta = reinterpret_cast<const uint2 *>(fam->set_meta);
  f.vpower32 = fam->vpower32;
  f.quorum = fam->quorum;
  f.vtab = fam->vtab;
  f.vslot_mask = fam->vslot_mask;
  f.n_union = fam->n_union;
  f.n_pieces = (int)np;
  const certd::proposer_table t{fam->t_height, fam->t_first, fam->t_addr20, fam->t_rounds};
  for (uint32_t v = 0; v < n_views && v < cap; v++) {
    wviews::view_t rec;
    wviews::view_record(rec, first_row[v], &acc[(size_t)v * (np + 1)], k, row_set, out_view, (int32_t)v, f, t, last_table, slots, salt);
    memcpy(out_views + (size_t)v * sizeof rec, &rec, sizeof rec);
  }
  return 0;
}

// the union's address table as ibft_set_validator_sets builds it: slots × 6 words {addr[5], index + 1}; → the slot mask
uint32_t wvh_build_vtab(const uint8_t *addrs20, uint32_t n_union, uint32_t *tab, uint32_t slots) {
  for (uint32_t i = 0; i < 6 * slots; i++) tab[i] = 0;
  for (uint32_t u = 0; u < n_union; u++) {
    uint32_t a[5];
    memcpy(a, addrs20 + 20ull * u, 20);
    uint32_t s = ibftk::addr_hash(a) & (slots - 1);
    while (tab[6 * s + 5]) s = (s + 1) & (slots - 1);
    memcpy(tab + 6 * s, a, 20);
    tab[6 * s + 5] = u + 1;
  }
  return slots - 1;
}

}  // extern "C"
