// host_cert_verdict_harness.hip — TEST-ONLY: cert_verdict_dev.h (the heads, the per-child steps and the folds of validPC and of
// the RoundChangeCertificate rules) on the CPU, so that tests/test_dev_cert_verdict_host.py can check the exact device source
// without a GPU.  cvh_judge walks the records the way cert_judge_kernel / cert_judge_children_kernel do, one child after the
// other instead of a lane each; distinct validators and power come from a validator-index column the test supplies.  Built
// with hipcc's host pass; never linked into libibftgpu.so, never a fallback.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <set>
#include <vector>

#include "cert_verdict_dev.h"

namespace {
constexpr int SUM_WORDS = 5;
void add_power(uint64_t acc[SUM_WORDS], const uint64_t *p, uint32_t pw) {
  unsigned __int128 carry = 0;
  for (int i = 0; i < SUM_WORDS; i++) {
    const unsigned __int128 t = (unsigned __int128)acc[i] + ((uint32_t)i < pw ? p[i] : 0) + carry;
    acc[i] = (uint64_t)t;
    carry = t >> 64;
  }
}
bool ge(const uint64_t a[SUM_WORDS], const uint64_t *b) {
  for (int i = SUM_WORDS - 1; i >= 0; i--)
    if (a[i] != b[i]) return a[i] > b[i];
  return true;
}
}  // namespace

extern "C" {

uint32_t cvh_record_size() { return (uint32_t)sizeof(certv::record); }

uint32_t cvh_pc_child(const wire::row_info *w, const wire::node_info *nd, uint8_t cls, int sender_bit, int hash_bit, int first, uint64_t height,
                      uint64_t limit, uint64_t ref_round, const uint8_t *ref_hash, int match_proposal) {
  const certv::pc_params p{height, limit, ref_round, ref_hash, match_proposal != 0};
  return certv::pc_child(*w, *nd, cls, sender_bit != 0, hash_bit != 0, first != 0, p);
}
uint32_t cvh_rcc_child(const wire::row_info *w, const wire::node_info *nd, uint8_t cls, int sender_bit, uint64_t height, uint64_t round) {
  return certv::rcc_child(*w, *nd, cls, sender_bit != 0, height, round);
}
int cvh_pc_fold(uint32_t flags, int all_distinct, int power_ok) { return certv::pc_fold(flags, all_distinct != 0, power_ok != 0); }
int cvh_rcc_fold(uint32_t flags, uint32_t n_children, int all_distinct, int power_ok) {
  return certv::rcc_fold(flags, n_children, all_distinct != 0, power_ok != 0);
}
int cvh_rcc_with_children(int rcc, int undecided) { return certv::rcc_with_children(rcc, undecided != 0); }
int cvh_pc_head(const wire::node_info *nodes, const wire::row_info *rows, const uint8_t *cls, uint32_t n_rows, uint32_t row, int match_proposal) {
  return certv::pc_head(nodes, rows, cls, n_rows, row, match_proposal != 0);
}
int cvh_rcc_head(const wire::node_info *nodes, const wire::row_info *rows, const uint8_t *cls, uint32_t n_rows, uint32_t row) {
  return certv::rcc_head(nodes, rows, cls, n_rows, row);
}

// The records of a tree of n_rows rows whose first n_roots are level 0.  sender / hash / self: one byte per row; vidx: the
// validator index of the row's From (−1: no member); power: n_validators × pw little-endian u64 words; quorum: 5 words.
// → number of records written to out (at most cap; more: −1).
int cvh_judge(const wire::node_info *nodes, const wire::row_info *rows, const uint8_t *cls, const uint8_t *sender, const uint8_t *hash,
              const uint8_t *self, uint32_t n_rows, uint32_t n_roots, const int32_t *vidx, const uint64_t *power, uint32_t pw,
              const uint64_t *quorum, certv::record *out, uint32_t cap) {
  std::vector<uint32_t> rec_row, first_cert(n_roots, certv::NO_RECORD);
  for (uint32_t r = 0; r < n_roots; r++) rec_row.push_back(r);
  for (uint32_t r = 0; r < n_roots; r++) {
    const uint32_t lo = nodes[r].first_child, n = nodes[r].n_children;
    if (n == 0 || (uint64_t)lo + n > n_rows || nodes[lo].role != wire::ROLE_RCC_MESSAGE) continue;
    first_cert[r] = (uint32_t)rec_row.size();
    for (uint32_t k = 0; k < n; k++) rec_row.push_back(lo + k);
  }
  if (rec_row.size() > cap) return -1;
  for (size_t rec = 0; rec < rec_row.size(); rec++) {
    const uint32_t row = rec_row[rec];
    const bool root = rec < n_roots;
    const wire::node_info &nd = nodes[row];
    const wire::row_info &ri = rows[row];
    const uint32_t parent = nd.parent;
    const uint64_t height = root ? ri.height : rows[parent].height, limit = root ? ri.round : rows[parent].round;
    int pc = certv::pc_head(nodes, rows, cls, n_rows, row, root);
    int rcc = root ? certv::rcc_head(nodes, rows, cls, n_rows, row) : certv::UNDECIDED;
    const bool walk_pc = pc == certv::GO, walk_rcc = rcc == certv::GO;
    uint32_t rcc_rows = 0;
    if (walk_pc || walk_rcc) {
      const uint32_t lo = nd.first_child, n = nd.n_children;
      certv::pc_params p{height, limit, 0, nullptr, root};
      if (walk_pc) {
        p.ref_round = rows[lo].round;
        p.ref_hash = rows[lo].proposal_hash;
      }
      uint32_t flags = 0, below = 0;
      std::set<int32_t> seen;
      uint64_t acc[SUM_WORDS] = {0, 0, 0, 0, 0};
      for (uint32_t c = lo; c < lo + n; c++) {
        flags |= walk_pc ? certv::pc_child(rows[c], nodes[c], cls[c], sender[c] != 0, hash[c] != 0, c == lo, p)
                         : certv::rcc_child(rows[c], nodes[c], cls[c], sender[c] != 0, ri.height, ri.round);
        below += 1 + nodes[c].n_children;
        if (!sender[c] || vidx[c] < 0 || !seen.insert(vidx[c]).second) continue;
        add_power(acc, power + (size_t)vidx[c] * pw, pw);
      }
      const bool all_distinct = seen.size() == n, power_ok = ge(acc, quorum);
      if (walk_pc) pc = certv::pc_fold(flags, all_distinct, power_ok);
      else {
        rcc = certv::rcc_fold(flags, n, all_distinct, power_ok);
        if (rcc != certv::UNDECIDED) rcc_rows = below;
      }
    }
    certv::record r;
    certv::record_head(r, row, nd, ri, cls[row], sender[row] != 0, hash[row] != 0, self[row] != 0);
    r.pc = (int8_t)pc;
    r.rcc = (int8_t)rcc;
    r.rcc_rows = rcc_rows;
    if (root) r.first_child_cert = first_cert[row];
    if (pc == certv::VALID) certv::record_pc_proposal(r, rows[nd.first_child]);
    out[rec] = r;
  }
  for (uint32_t root = 0; root < n_roots; root++) {
    certv::record &r = out[root];
    if (r.rcc != certv::VALID || r.first_child_cert == certv::NO_RECORD) continue;
    bool undecided = false;
    for (uint32_t k = 0; k < r.n_children; k++) undecided = undecided || out[r.first_child_cert + k].pc == certv::UNDECIDED;
    r.rcc = (int8_t)certv::rcc_with_children(certv::VALID, undecided);
  }
  return (int)rec_row.size();
}

}  // extern "C"
