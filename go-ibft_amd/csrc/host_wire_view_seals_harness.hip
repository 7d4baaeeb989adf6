// host_wire_view_seals_harness.hip — TEST-ONLY: the row bodies of the wire_seals_*_kernel launches (wire_seals_dev.h) and the
// seal form of the views stage (wire_views_dev.h) on the CPU, so that tests/test_dev_wire_view_seals_host.py can check the exact
// device source without a GPU: the sealable decision with its membership lookup, the dense order of the seal rows, how a seal
// verdict and the final sender bit become a row's seal bit, and the records tallied over stored ∧ sealed.  The cross-row parts
// — the scans, the sums — are plain loops here where the kernels have their workgroup scans and their wavefront turns.  Built
// with hipcc's host pass; never linked into libibftgpu.so, never a fallback.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "wire_seals_dev.h"

extern "C" {

struct wsh_family {  // (host_wire_views_harness.hip: wvh_family)
  const int32_t *setidx;
  const uint32_t *set_meta, *vpower32;
  const uint64_t *quorum;
  const uint32_t *vtab;
  uint32_t vslot_mask, n_union, n_pieces;
  uint64_t t_height, t_first;
  const uint8_t *t_addr20;
  uint32_t t_rounds;
};

static wviews::family family_of(const wsh_family *fam) {
  wviews::family f;
  f.setidx = fam->setidx;
  f.set_meta = reinterpret_cast<const uint2 *>(fam->set_meta);
  f.vpower32 = fam->vpower32;
  f.quorum = fam->quorum;
  f.vtab = fam->vtab;
  f.vslot_mask = fam->vslot_mask;
  f.n_union = fam->n_union;
  f.n_pieces = (int)fam->n_pieces;
  return f;
}

// mark + scan: n parsed rows (80 bytes each) and their sets → flags (wseals::ROW_*), seal_row[i] (k or NONE), src[k];
// counts[0] = sealable rows, counts[1] = COMMIT rows with a set
void wsh_stage(const uint8_t *rows80, const int32_t *row_set, uint32_t n, const wsh_family *fam, uint8_t *flags, uint32_t *seal_row,
               uint32_t *src, uint32_t *counts) {
  const wire::row_info *rows = reinterpret_cast<const wire::row_info *>(rows80);
  const wviews::family f = family_of(fam);
  uint32_t run = 0, commits = 0;
  for (uint32_t i = 0; i < n; i++) {
    flags[i] = wseals::row_flags(rows[i], row_set[i], f);
    commits += (flags[i] & wseals::ROW_COMMIT) ? 1u : 0u;
    const bool sealable = flags[i] & wseals::ROW_SEALABLE;
    seal_row[i] = sealable ? run : wseals::NONE;
    if (sealable) src[run++] = i;
  }
  counts[0] = run;
  counts[1] = commits;
}

// combine: valid[i] = the final sender bit, seal_words = the verdict words of the seal half → the seal mask (⌈n/64⌉ words)
void wsh_combine(const uint8_t *valid, const uint32_t *seal_row, uint32_t n, const uint64_t *seal_words, uint64_t *out_seal) {
  for (uint32_t w = 0; w < (n + 63) / 64; w++) out_seal[w] = 0;
  for (uint32_t i = 0; i < n; i++)
    if (wseals::seal_bit(valid[i] != 0, seal_row[i], seal_words)) out_seal[i >> 6] |= 1ull << (i & 63);
}

// The views stage in its seal form over n parsed rows, as wvh_run (host_wire_views_harness.hip) runs the plain one; seal: the
// rows' seal bits (⌈n/64⌉ words).  → 0, or 1 when a table was exhausted.
int wsh_run(const uint8_t *rows80, const int32_t *vidx, const int32_t *row_set, const uint8_t *valid, const uint64_t *seal, uint32_t n,
            uint32_t slots, uint32_t salt, uint32_t views_cap, const wsh_family *fam, int32_t *out_view, uint64_t *out_stored, uint8_t *out_views,
            uint32_t *out_n_views) {
  const wire::row_info *rows = reinterpret_cast<const wire::row_info *>(rows80);
  const wviews::columns k{rows, vidx};
  std::vector<uint32_t> tables(2 * (size_t)slots, wviews::EMPTY);
  uint32_t *key_table = tables.data(), *last_table = tables.data() + slots;
  std::vector<wviews::row_slots> sl(n);
  for (uint32_t r = 0; r < n; r++) {
    sl[r] = wviews::insert_row(k, r, valid[r] != 0, key_table, last_table, slots, salt);
    if (sl[r].key == wviews::UNPLACED || sl[r].last == wviews::UNPLACED) return 1;
  }
  std::vector<uint32_t> rank_of(n, 0), first_row;
  for (uint32_t r = 0; r < n; r++)
    if (wviews::is_rep(key_table, sl[r].key, r)) {
      rank_of[r] = (uint32_t)first_row.size();
      first_row.push_back(r);
    }
  const uint32_t n_views = (uint32_t)first_row.size();
  *out_n_views = n_views;
  const uint32_t np = fam->n_pieces, cap = views_cap < n ? views_cap : n, stride = np + 2;
  std::vector<uint64_t> acc((size_t)cap * stride + 1, 0);
  for (uint32_t w = 0; w < (n + 63) / 64; w++) out_stored[w] = 0;
  for (uint32_t r = 0; r < n; r++) {
    out_view[r] = wviews::VIEW_NONE;
    if (sl[r].key >= wviews::SKIP) continue;
    const int32_t v = wviews::view_of_rank(rank_of[key_table[sl[r].key]], cap);
    const bool stored = wviews::is_stored(last_table, sl[r].last, r);
    out_view[r] = v;
    if (stored) out_stored[r >> 6] |= 1ull << (r & 63);
    if (v < 0) continue;
    uint64_t *a = &acc[(size_t)v * stride];
    a[np] += 1ull | ((uint64_t)(stored ? 1u : 0u) << 32);
    const bool sealed = (seal[r >> 6] >> (r & 63)) & 1ull;
    if (wseals::counts(rows[r].type, stored, sealed)) {
      const uint32_t entry = reinterpret_cast<const uint2 *>(fam->set_meta)[row_set[r]].x + (uint32_t)vidx[r];
      for (uint32_t i = 0; i < np; i++) a[i] += fam->vpower32[(size_t)entry * np + i];
      a[np + 1] += 1;
    }
  }
  const wviews::family f = family_of(fam);
  const certd::proposer_table t{fam->t_height, fam->t_first, fam->t_addr20, fam->t_rounds};
  for (uint32_t v = 0; v < n_views && v < cap; v++) {
    wviews::view_t rec;
    wviews::view_record(rec, first_row[v], &acc[(size_t)v * stride], k, row_set, out_view, (int32_t)v, f, t, last_table, slots, salt, true);
    memcpy(out_views + (size_t)v * sizeof rec, &rec, sizeof rec);
  }
  return 0;
}

}  // extern "C"
