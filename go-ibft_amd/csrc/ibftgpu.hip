// ibftgpu.hip — host side of libibftgpu.so: the C ABI declared in include/ibftgpu.h.
//
// Product code.  No CPU verification path exists here on purpose: if the device or a
// HIP call fails the entry point returns a negative code and the caller (the Go shim,
// INTEGRATION.md) runs its own per-message Verifier for that batch.
#include "../../include/ibftgpu.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl is dlopen()ed on first use (ibft_comm_* / ibft_group_*)
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <thread>
#include <unordered_map>
#include <string>
#include <vector>

#include "kernels.hip.h"

namespace {

constexpr uint32_t DEFAULT_MAX_ROWS = 65536;

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
};
void release(DevBuf &b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

}  // namespace

// What belongs to a DEVICE rather than to a context: the fixed-base table of G (84 MB, 9 ms to build) and — with
// IBFT_FLAG_PUBKEY_CACHE — the validators' key tables.  Every context of a device shares one copy (the four contexts a
// Backend holds for its four goroutines, the several ranks of a group that lists one device more than once); the tables
// are keyed by ADDRESS, so a validator keeps its slot and its table when the validator set changes around it.
struct KeyAddr {
  uint8_t b[20];
  bool operator==(const KeyAddr &o) const { return memcmp(b, o.b, 20) == 0; }
};
struct KeyAddrHash {
  size_t operator()(const KeyAddr &a) const {
    uint64_t x, y;
    uint32_t z;
    memcpy(&x, a.b, 8);
    memcpy(&y, a.b + 8, 8);
    memcpy(&z, a.b + 16, 4);
    return (size_t)((x * 0x9E3779B97F4A7C15ull) ^ (y * 0xC2B2AE3D27D4EB4Full) ^ z);
  }
};
struct DeviceShared {
  std::mutex mu;  // taken around every launch that reads the pointers below and around every change of them
  int device = 0;
  DevBuf d_gtab;
  // key cache: slot s holds pub (80 B), state (0 unknown, 1 key known, 2 table built) and a table of slot_bytes: 655 360 B in
  // the wide form, 174 080 B in the GLV form (verify_dev.h).  The pool is one array of equal slots shared by every context, so
  // the form is the POOL's: IBFT_QTAB_FORM=wide|glv, read once, when this object is created.
  int form = ibftk::QTAB_WIDE;
  size_t slot_bytes = (size_t)ibftk::QTAB_DWORDS_PER_VALIDATOR * 4;
  DevBuf d_pub, d_state, d_qtab, d_learned;  // d_learned: {keys learned, a learned slot} (two u32), bumped by the kernels
  uint32_t cap = 0;                          // slots allocated
  std::unordered_map<KeyAddr, uint32_t, KeyAddrHash> slot_of;
  std::vector<uint32_t> refs;                // contexts whose current validator set holds the slot's address
  std::vector<KeyAddr> addr_of;
  std::vector<uint8_t> built;                // host shadow of state == 2 (refreshed after every build pass)
  std::vector<uint32_t> free_slots;
  uint32_t used = 0;                         // slots handed out so far (high-water mark)
  uint32_t learned_seen = 0;                 // value of the device counter up to which tables are built (or being built)
  uint32_t dummy_slot = 0;
  uint64_t build_epoch = 1;                  // bumped by every build pass: contexts recount their built validators
  uint64_t generation = 1;                   // bumped when the buffers move: contexts re-read the pointers
};
std::mutex g_devices_mu;
std::map<int, std::weak_ptr<DeviceShared>> g_devices;
// why the calling thread's last ibft_ctx_create failed, "" after one that succeeded (ibft_last_error(NULL)): per thread, so a
// create failing on another thread never touches the string a reader holds
thread_local std::string g_create_error;
// IBFT_QTAB_FORM → the table form; -1 for a value that is neither
int qtab_form_from_env() {
  const char *e = getenv("IBFT_QTAB_FORM");
  if (!e || !strcmp(e, "wide")) return ibftk::QTAB_WIDE;
  if (!strcmp(e, "glv")) return ibftk::QTAB_GLV;
  return -1;
}

// A FAMILY of validator sets (ibft_set_validator_sets): state of its own next to the context's single set.  The first block
// of members is what the verdict kernels and the key cache know as "the validator set" — one table over the UNION of the
// family's addresses, the union's key-cache slots; while a _sets call runs these are exchanged with the context's own
// (family_view), so enqueue_recover, build_new_tables and the key cache serve both without knowing which they serve.  The
// rest is what only the sets form of block_tally_kernel reads.
struct ValFamily {
  DevBuf d_vtab, d_vslot;
  std::vector<uint32_t> vslot;
  uint32_t vslot_mask = 0, n_union = 0, my_built = 0;
  uint64_t seen_build_epoch = 0;
  bool cache_on = false;

  bool have = false;
  uint32_t n_sets = 0, power_words = 1, largest_set = 0;
  uint32_t entries = 0;  // Σ distinct addresses over the sets: entries of d_power, bits of the wire route's bitmap
  DevBuf d_setidx, d_meta, d_power, d_quorum, d_seen, d_bset;
  std::vector<uint64_t> quorum;  // n_sets × TALLY_SUM_WORDS
  uint64_t device_bytes = 0;
};

// The per-block records of a block batch, one 4-word record per block: the tally delivers them into mapped pinned host memory
// where the device can write it (h, through map; grown on demand), through d and a copy behind the tally otherwise.
struct BlockRecords {
  DevBuf d;
  uint64_t *h = nullptr, *map = nullptr;
  size_t blocks = 0;
};
// One of the two slots of the streamed chain sync (ibft_block_seals_submit … / _collect): everything a batch in flight reads
// and delivers beyond the verdict words, PRIVATE to its slot, so that the kernels of batch k + 1 never write what batch k
// still has to deliver.  All of it is free again when batch k − 2 has been collected.
struct BlockSlot {
  BlockRecords rec;
  uint32_t rows = 0, blocks = 0, kind = 0;  // kind: IBFT_BATCH_* of the batch (0 for a batch of ibft_block_seals_submit)
  uint64_t quorum[2] = {0, 0};       // the quorum a batch was judged under (the set current at its submit)
  // the proposals as given (bytes with 256 of slack, offsets, rounds: two slots double the device bytes proposals take, each
  // slot bounded by IBFT_PROPOSAL_BYTES_MAX), the blocks' digests (computed, or the uploaded hashes of a hashes-given batch)
  // that block_head_kernel reads and never writes, and for a recover batch the columns the emitting kernels fill — swapped
  // in for d_signer_out / d_vidx while the batch's kernels are enqueued (emit_columns_view)
  DevBuf praw, proff, pround, phash, signer, vidx;
  // … and the page-locked buffers digests, signers and indices come back into, on ostream: behind ev_dig (the digests exist)
  // and ev (the tally is done); ev_out is behind the last copy, and the collect waits for it when has_out says there was one
  uint8_t *h_hash = nullptr, *h_signer = nullptr;
  int32_t *h_vidx = nullptr;
  size_t h_hash_blocks = 0, h_rows = 0, h_vidx_rows = 0;
  hipEvent_t ev = nullptr, ev_dig = nullptr, ev_out = nullptr;
  bool has_out = false;
  // A batch judged under a family of sets (the _sets submits, IBFT_BATCH_SETS in kind): its block_set column lies in a buffer
  // of the SLOT — the copy of batch k + 1 must not overwrite what the tally of batch k reads, so fam.d_bset will not do — and
  // the quorum words its collect hands out are kept on the host, so that what the collect DELIVERS never comes from c->fam
  // (the family may have been replaced since; only the table build behind the delivery counts against the union installed
  // then): setq holds the two low quorum words per BLOCK when setidx is empty, per SET of the family of the submit when
  // setidx holds the blocks' set indices — whichever of the two is smaller for the batch.
  DevBuf bset;
  std::vector<uint64_t> setq;
  std::vector<uint32_t> setidx;

  void release_all() {  // device buffers, pinned buffers, events: everything the slot owns (ibft_ctx_destroy)
    for (DevBuf *b : {&rec.d, &praw, &proff, &pround, &phash, &signer, &vidx, &bset}) release(*b);
    for (void *h : {(void *)rec.h, (void *)h_hash, (void *)h_signer, (void *)h_vidx})
      if (h) (void)hipHostFree(h);
    for (hipEvent_t e : {ev, ev_dig, ev_out})
      if (e) (void)hipEventDestroy(e);
  }
  uint64_t block_set_bytes() const { return bset.cap; }  // (ibft_validator_sets_info)
};

// The counter block of a certificate call, 64 bytes: once in HBM (CertState::total), once in pinned memory (h_total; dh_total
// is that mirror as the device sees it).  The kernels keep their word pointers — each is handed the address of the first
// field it writes — and the host reads the fields by name.
struct cert_counters {
  uint32_t next_rows, carriers;  // cert_scan_launch, once per level: rows of the next level, deferred rows among this level's
  uint32_t records;              // cert_record_scan_kernel (judge, when level 1 is listed): rows that get a record
  uint32_t pad0;
  uint32_t dense, unplaced;               // cert_dedup_front_launch: representatives, rows the table could not place
  uint32_t judged_tree, judged_deferred;  // cert_dedup_count_launch: rows without a pre-flag, the tree's and the deferred batch's
  uint32_t count_acc[3];                  // cert_dedup_count_kernel's two sums and its ticket: zero between launches
  // the round-change stage's three words (pinned mirror only: copied there from behind the stage's tables): keys, all-ones unless a
  // table was exhausted, unjudged level-0 rows
  uint32_t rc_words[3];
  uint32_t pad1[2];
};
static_assert(sizeof(cert_counters) == 64, "the counter block the kernels address by word");
static_assert(offsetof(cert_counters, next_rows) == 0 && offsetof(cert_counters, carriers) == 4 && offsetof(cert_counters, records) == 8 &&
                  offsetof(cert_counters, pad0) == 12 && offsetof(cert_counters, dense) == 16 && offsetof(cert_counters, unplaced) == 20 &&
                  offsetof(cert_counters, judged_tree) == 24 && offsetof(cert_counters, judged_deferred) == 28 &&
                  offsetof(cert_counters, count_acc) == 32 && offsetof(cert_counters, rc_words) == 44 && offsetof(cert_counters, pad1) == 56,
              "cert_scan_launch writes words 0-1, cert_record_scan_kernel word 2, the dedup front words 4-5, the count launch 6-7 over 8-10");

// Certificates from wire bytes (ibft_verify_certificates_wire, ibft_judge_certificates_wire): everything the route owns beyond
// the shared columns, grown by the first call that needs it (cert_reserve) and kept.
struct CertState {
  // tree nodes, where each row's nested messages lie, child counts of the level being expanded, the deferred rows' list,
  // proposal digests, hash / self words, the tile scan's cells; the counters come back through one mapped block
  DevBuf nodes, span, count, slot, prop, masks, total, tiles;
  DevBuf rec, recbase;            // ibft_judge_certificates_wire: one record per carrier, the roots' first records
  DevBuf dd_table, dd_slot, dd_pos;  // the dedup: the table, every row's slot, every representative's dense position
  // ibft_decide_certificates_wire: one decision per record, the roots' sponge states behind the full blocks of their proposals;
  // ibft_set_proposers: the proposers of rounds [prop_first, prop_first + prop_rounds) of prop_height (room for the most, once)
  DevBuf dec, mid, proposers;
  uint64_t prop_height = 0, prop_first = 0;
  uint32_t prop_rounds = 0;
  cert_counters *h_total = nullptr, *dh_total = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;  // the side stream (hstream) hashes the deferred rows next to the verdict launch
  bool overlap = true;                              // IBFT_CERT_OVERLAP=0: everything on one stream, one verdict launch
  // IBFT_FLAG_CERT_DEDUP / IBFT_CERT_DEDUP=0|1: the (first) verdict launch of a certificate call judges each distinct
  // (digest, signature, From) once (cert_dedup_dev.h)
  bool dedup = false;
  uint32_t dedup_slots_cap = 0;     // IBFT_CERT_DEDUP_SLOTS (test hook): at most that many table slots; 0 = no cap
  uint32_t stat[4] = {0, 0, 0, 0};  // ibft_cert_stats: rows, judged, given to the verdict kernels, unplaced — of the last certificate call
  // ibft_decide_round_changes_wire (kernels.hip.h: round_change_*_kernel), sized by n and rc_cap in the call itself, in the
  // views call's discipline: the two tables with the call's three words behind them (2 · slots + 4 words, set to all-ones by
  // ONE fill in front of every insert), the rows' sender indices, slots, ranks and views, the stored words, the records, the
  // answer, and the per-key accumulators, which every successful call leaves zero (rc_acc_dirty: a call that failed midway may
  // not have; the next one clears them first).
  DevBuf rc_tables, rc_slots, rc_vidx, rc_rank, rc_first, rc_view, rc_stored, rc_acc, rc_recs, rc_answer;
  bool rc_acc_dirty = true;
  uint32_t rc_slots_hook = 0;  // IBFT_ROUND_CHANGE_SLOTS (test hook): lowers the slot count, never below the first power of two above n

  void release_all() {  // device buffers, the pinned block, the two events (ibft_ctx_destroy)
    for (DevBuf *b : {&nodes, &span, &count, &slot, &prop, &masks, &total, &tiles, &rec, &recbase, &dd_table, &dd_slot, &dd_pos, &dec, &mid, &proposers,
                      &rc_tables, &rc_slots, &rc_vidx, &rc_rank, &rc_first, &rc_view, &rc_stored, &rc_acc, &rc_recs, &rc_answer})
      release(*b);
    if (h_total) (void)hipHostFree(h_total);
    for (hipEvent_t e : {ev_fork, ev_join})
      if (e) (void)hipEventDestroy(e);
  }
};

// What the flat wire calls left in the columns: `rows` rows of the last ibft_verify_senders_wire / ibft_verify_messages_wire.
// One count serves both flags: only ibft_verify_senders_wire sets `columns`, and whatever sets `parsed` after it either is
// that same call or has cleared `columns` on its way in.
struct WireBatch {
  uint32_t rows = 0;
  bool columns = false;  // ibft_wire_stage_seals: the senders-wire batch is still the resident one
  bool parsed = false;   // ibft_wire_stats: its parse results are still in d_wire_rows
  // ibft_wire_seal_stats: the two counts of the last ibft_verify_messages_wire_views (zero once any other wire call has begun)
  uint32_t commit_rows = 0, seal_rows = 0;
  void begin() {  // a wire call takes the columns over
    parsed = false;
    commit_rows = seal_rows = 0;
  }
};

// The height map of the live route under a family (ibft_set_height_sets) and what ibft_verify_senders_wire_sets keeps next to
// the shared columns: the rows' sets, the per-set accumulators and the (set, member) bitmap of wire_sets_tally_kernel — both
// sized for the family the map was installed under, zeroed then, and left zero by every launch.  The map's indices name sets
// of THAT family: installing a family drops the map.
struct HeightSets {
  bool have = false;
  uint32_t n_ranges = 0;
  uint64_t lo = 0, hi = 0;  // first_height[0], first_height[n_ranges]
  DevBuf d_first, d_range_set, d_row_set, d_acc, d_seen;
};

// What ibft_verify_senders_wire_views keeps behind the sets call's columns (kernels.hip.h: wire_views_*_kernel), sized lazily by
// n and views_cap in the call itself: the two tables with the call's two words behind them (2 · slots + 2 words, set to all-ones
// — EMPTY, "no error" — by ONE fill in front of every insert), the rows' slots, ranks and views, the stored words, and the
// per-view accumulators, which every successful call leaves zero (acc_dirty: a call that failed midway may not have; the next
// one clears them first).
// ibft_verify_messages_wire_views adds, allocated by its first call: the rows' flags, seal rows and their source rows, the
// call's three words (kernels.hip.h: wire_seals_args) and the seal mask.  Its accumulators are one word per view longer — the
// same buffer, zero between calls whichever of the two calls ran.
struct WireViews {
  DevBuf d_tables, d_slots, d_rank, d_first, d_view, d_stored, d_acc, d_recs;
  DevBuf d_sflags, d_seal_row, d_seal_src, d_seal_words, d_seal_mask;
  bool acc_dirty = true;
  uint32_t salt = 0;        // per context, from the system's entropy: nobody outside can aim rows at one probe run
  uint32_t slots_hook = 0;  // IBFT_WIRE_VIEWS_SLOTS (test hook): lowers the slot count, never below the first power of two above n
};

struct ibft_ctx {
  std::mutex mu;
  std::shared_ptr<DeviceShared> dev;   // the G table and the key cache of this context's device
  DevBuf d_vslot;                      // validator index → key-cache slot (0xFFFFFFFF = none)
  std::vector<uint32_t> vslot;         // the same on the host
  uint32_t my_built = 0;               // validators of the current set whose table is built
  uint64_t seen_build_epoch = 0;
  int device = 0;
  uint32_t flags = 0;
  uint32_t max_rows = DEFAULT_MAX_ROWS;
  uint32_t row_cap = 0;  // rows the columns can hold: max_rows, or 2·⌈max_rows/64⌉·64 once a message set was verified
  uint32_t kernel = IBFT_KERNEL_AUTO;
  hipStream_t stream = nullptr;
  std::string last_error;

  // columns in HBM
  DevBuf d_hash, d_sig, d_signer, d_pre, d_hash_len, d_payload, d_off, d_raw;
  DevBuf d_signer_out;  // the address column the emitting cold kernels write (ibft_recover_seals / ibft_recover_block_seals)
  DevBuf d_msg_cols, d_msg_wire;  // ibft_sign_messages_wire: height ‖ round ‖ type columns in, the wire bytes out
  DevBuf d_env_cols, d_env_body, d_env_wire;  // ibft_sign_envelopes_wire: the row columns, the bodies in, the wire bytes out (grown on demand, kept)
  // the SECOND staging slot of the seal columns (ibft_seals_stage_next / ibft_seals_swap): batch k+1 is copied here on a
  // copy stream of its own while the verdict kernels read batch k from the columns above; a swap exchanges the two sets
  DevBuf d_hash_nx, d_sig_nx, d_signer_nx, d_pre_nx;
  hipStream_t cstream = nullptr;
  hipEvent_t ev_staged = nullptr, ev_cols_read = nullptr;  // the copy into the spare slot is done / the spare slot's last reader is
  uint32_t next_n = 0;
  bool next_pre = false, next_valid = false;
  // pipelined passes (ibft_seals_submit / ibft_seals_collect): two host-visible result slots, an event behind each pass's tally
  uint64_t *p_mask[2] = {nullptr, nullptr}, *p_tally[2] = {nullptr, nullptr}, *dp_mask[2] = {nullptr, nullptr}, *dp_tally[2] = {nullptr, nullptr};
  hipEvent_t ev_pass[2] = {nullptr, nullptr};
  uint32_t pass_issued = 0, pass_collected = 0, pass_n[2] = {0, 0};
  int learn_rc = IBFT_OK;  // a table build behind a DELIVERED pass failed: reported by the next ibft_seals_submit
  bool split_large = true;    // batches of 65 537 … 98 304 rows as two launches (enqueue_recover); IBFT_SPLIT_LARGE=0 turns it off (A/B)
  uint32_t split_launches = 0;
  int tally_slot = -1;      // ≥ 0: the next tally delivers into pipeline slot `tally_slot` instead of h_mask / h_tally
  // The tally of a pipelined pass on a stream of its own (round 6): pass k's tally (one small workgroup, 9–15 µs with its
  // dependency gap) runs NEXT TO pass k + 1's verdict kernel instead of in front of it.  What the two would share is doubled:
  // the work mask and the validator-index column exist twice (d_mask / d_vidx are the pair the next verdict launch writes,
  // d_mask_b / d_vidx_b the pair the tally in flight reads and zeroes; ibft_seals_submit swaps them), and pair P(k) = P(k − 2) is
  // free again because pass k − 2 was collected before pass k could be submitted (at most two in flight).  Every OTHER entry
  // point puts the main stream behind the side stream's tallies first (ctx_lock → join_side).
  // MEASURED (profiles/r06v…r06y_side_tally_ab.txt, r06v_side_tally_trace.txt).  Two things had to be learned: (1) the tally
  // must FIT next to a resident verdict kernel — the one-workgroup form (sixteen wavefronts of 126 registers) fits next to
  // nothing and simply waited for the NEXT verdict kernel to end (N = 4 096: 0.351 → 0.505 ms per step); the ticket form (42
  // registers) does, so a side-stream tally always takes that one (enqueue_tally); (2) the lane / group cold kernels fill the
  // LDS of every compute unit with their window tables: a tally workgroup placed first takes the room of a verdict workgroup,
  // which then runs as a second round (N = 16 384: 0.71 → 1.37 ms, 65 536: 0.92 → 1.87).  Behind everything else it pays:
  // cold N = 64 … 8 192 −0.8 … −1.7 % per step, warm N = 1 024 … 65 536 −2.3 … −6 %.  Hence side_tally: 0 never, 1 always
  // (A/B), 2 = AUTO (ibft_seals_submit).  IBFT_SIDE_TALLY=0|1 pins it.
  int side_tally = 2;
  bool side_pending = false;
  hipStream_t tstream = nullptr;
  hipEvent_t ev_rec[2] = {nullptr, nullptr};   // pass k's verdict kernels are done (recorded on the stream that carried them)
  DevBuf d_mask_b, d_vidx_b;
  uint32_t mask_dirty_words_b = ~0u;
  uint32_t side_tallies = 0;                   // passes whose tally ran on the side stream (ibft_last_dispatch-style counter)
  // Pipelined passes on two verdict streams (round 21): consecutive ibft_seals_submit passes put their verdict launch (mask
  // clearing, warm and cold stage, the event pair of a timed pass) alternately on the main stream and on hstream — idle while
  // the pipeline runs — so that pass k + 1 may start in the tail of pass k instead of behind it.  The pass's tally follows an
  // event on the stream that carried its verdict launch, and ev_pass[s] is behind that tally: whoever waits for both ev_pass
  // (join_side) is behind everything either verdict stream carries.  0 never, 1 wherever the side-stream tally's conditions
  // hold (A/B, tests), 2 = AUTO (alt_verdict_applies); IBFT_ALT_VERDICT=0|1 pins it.  DESIGN §5.10.
  int alt_verdict = 2;
  bool last_on_alt = false;                    // the pass submitted last took hstream
  // the main stream may carry work since hstream last waited for it that a verdict launch on hstream must not overtake: any
  // entry point outside the pipeline (ctx_lock), a tally the pipeline left on the main stream, a digest pass behind a swap
  bool main_touched = true;
  bool alt_used = false;                       // hstream has carried a verdict launch (what a timing read / a swap must cover)
  uint32_t alt_passes = 0;                     // passes whose verdict launch took hstream (ibft_pipeline_stats_ex)
  hipEvent_t ev_cols_read_b = nullptr;         // ev_cols_read's twin on hstream
  uint32_t launched_n = 0;  // rows of the last ibft_seals_launch: what ibft_seals_fetch delivers (a swap may have changed staged_n since)
  DevBuf d_mask, d_vidx, d_tally, d_H;
  DevBuf d_mask_out;        // verdict words after the tally consumed d_mask (what fetch / export read)
  // d_mask words [0, mask_dirty_words) may hold bits; 0 = the whole work mask is zero (the tally left it so)
  // and no memset is needed in front of the atomicOr kernels
  uint32_t mask_dirty_words = ~0u;
  DevBuf d_wire_rows, d_seal;  // §8f rank 3: per-row parse results and the COMMIT seals found in the wire bytes
  DevBuf d_noseal;             // message sets from wire bytes: rows (PREPAREs) whose closure has no seal
  WireBatch wire;              // what the last flat wire call left resident
  // IBFT_FLAG_WIRE_RECODE / IBFT_WIRE_RECODE=0|1: the flat wire calls run wire_recode_kernel over the rows the canonical walk
  // marked NEEDS_HOST (wire_recode_dev.h)
  bool wire_recode = false;
  // fixed-base table for G
  // validator table
  DevBuf d_vtab, d_vpower;
  uint32_t vslot_mask = 0;
  uint32_t n_validators = 0;
  bool have_valset = false;
  uint32_t power_words = 1;                          // 64-bit words per voting power: 1 (u64) or 4 (256-bit)
  uint64_t quorum_w[ibftk::TALLY_SUM_WORDS] = {0};   // ⌊2·total/3⌋+1, little-endian words
  DevBuf d_seen, d_acc, d_quorum;                    // tally: distinct-sender bitmap, launch-wide sums + ticket, quorum words
  // chain sync (ibft_verify_block_seals): the blocks' hashes and row offsets, and the records of the synchronous calls
  DevBuf d_bhash, d_boff;
  BlockRecords brec;
  // Streamed chain sync (ibft_block_seals_submit / _collect): at most two batches in flight.  Batch k is copied on the copy
  // stream into the SPARE column set — d_sig_nx / d_signer_nx / d_pre_nx of the seal pipeline plus a second offset buffer —
  // while the kernels of batch k − 1 read the resident set; the submit then swaps the two sets, exactly as
  // ibft_seals_stage_next + ibft_seals_swap would (ev_cols_read: the spare set's last reader, ev_staged: the copy landed).
  // Every kernel of a batch runs on the MAIN stream: the per-row hash column block_head_kernel fills, the work mask, the
  // validator indices, d_seen and the ticket word in d_acc exist once and rely on that order — and any other entry point that
  // enqueues on the main stream is behind the batches in flight by the same order, their results already on the way to
  // their slots.  Results: verdict words in the seal pipeline's mapped slots (p_mask; the two pipelines are never mixed),
  // {keys learned, a learned slot} in p_tally[s][4], everything else in bs[s] (BlockSlot).  Digests, signers and indices come
  // back on ostream — NOT the copy stream, whose next command is the upload of batch k + 1 and must not wait for batch k's
  // tally.  ostream and the slots' events are created by the first submit of ANY kind: a context that only ever calls
  // ibft_block_seals_submit has them too and never puts a command on ostream.
  DevBuf d_boff_nx;
  BlockSlot bs[2];
  uint32_t bs_issued = 0, bs_collected = 0;
  hipStream_t ostream = nullptr;
  bool stream_digest_copy = false;  // IBFT_STREAM_DIGEST=copy|main: the stream proposal_digest_kernel of a streamed batch runs on
  // Chain sync from the proposals (ibft_proposal_hashes, the _raw block calls): the caller's proposals as they are — bytes,
  // offsets, rounds — in buffers of their own (grown on demand and kept, like d_payload; the bytes carry 256 of slack), the n
  // digests proposal_digest_kernel writes (what block_head_kernel then reads in place of an uploaded d_bhash), and the pinned
  // mirror the digests come back through.  None of it is the remembered proposal of ibft_proposal_hash (d_H, hashed_proposal).
  DevBuf d_praw, d_proff, d_pround, d_phash;
  uint8_t *h_phash = nullptr;
  size_t h_phash_rows = 0;
  uint64_t proposal_bytes_max = 256ull << 20;  // IBFT_PROPOSAL_BYTES_MAX: the most raw_off[n] may be (IBFT_E_TOOBIG beyond)
  uint32_t proposal_lanes_force = 0;           // IBFT_PROPOSAL_LANES=1|64 pins the form of proposal_digest_kernel (tests, A/B)
  uint32_t envelope_lanes_force = 0;           // IBFT_ENVELOPE_LANES=1|64 pins the form of envelope_digest_kernel (tests, A/B)
  uint32_t proposal_lane_rows = 8192;          // AUTO: the lane form from this many proposals of the longest one's length on
  ValFamily fam;                                     // ibft_set_validator_sets / the _sets block calls
  HeightSets hsets;                                  // ibft_set_height_sets / ibft_verify_senders_wire_sets
  WireViews wviews;                                  // ibft_verify_senders_wire_views
  uint64_t valsets_bytes_max = 512ull << 20;         // IBFT_VALSETS_BYTES_MAX: the most a family's device tables may take
  uint64_t last_wide[ibftk::TALLY_SUM_WORDS] = {0};  // full-width power of the last fetched tally
  uint64_t height = 0;
  // the seal-digest convention of the embedding Backend (ibft_set_seal_digest): 0 = the proposalHash itself
  uint32_t seal_digest_mode = 0;
  uint64_t seal_suffix_words[9] = {0};
  DevBuf d_hash_copy;            // message sets under a non-identity convention: the carried hashes a1 compares
  std::vector<uint32_t> h_vtab;  // host copy of the validator table (6 dwords per slot): the proposer's seat is looked up here
  // HasPrepareQuorum: set by an entry point that was given a proposer, consumed by the next tally it enqueues
  bool next_prop_on = false;
  int32_t next_prop_vidx = -1;
  // … and that tally is ONE SHARD's share of a sharded PREPARE set whose exchange follows in the same call (set by
  // ibft_group_verify_messages only): the proposer's seat is then left to the merge.  Every other tally — ibft_tally_prepare,
  // a one-shot ibft_verify_messages[_wire] — adds the seat itself, also on a context that is a member of a group or of a
  // communicator (round-4 advice: the seat was dropped by membership, and HasPrepareQuorum under-counted there).
  bool next_shard = false;
  uint32_t last_proposer_rows = 0;

  // multi-GPU exchange (ibft_comm_*): rows of a batch sharded over `xworld` contexts, one all-reduce merges them
  ncclComm_t comm = nullptr;
  bool xlocal = false;  // a rank of a group whose collective is the library's own sum kernel (no communicator)
  uint32_t xrank = 0, xworld = 1;
  hipStream_t xstream = nullptr;
  DevBuf d_xbuf[2], d_xres[2];
  DevBuf d_seen_out;    // the last tally's distinct-sender bitmap (⌈n_validators/64⌉ u64 words): what the ranks exchange
  hipEvent_t ev_xpack = nullptr;  // local collective: this rank's buffer is packed / the summed buffers are back
  uint32_t x_K[2] = {1, 1};       // verdict arrays of the exchange in each slot (1: seal / sender batch, 2: message set)
  uint32_t set_n = 0;             // rows of the last message set (its words are in d_set)
  uint64_t *h_xres[2] = {nullptr, nullptr}, *dh_xres[2] = {nullptr, nullptr};
  size_t h_xres_words = 0;
  hipEvent_t ev_xdone[2] = {nullptr, nullptr};
  uint64_t x_total[2] = {0, 0};   // n_total of the exchange in each slot
  uint32_t x_issued = 0, x_fetched = 0;  // exchanges enqueued / consumed (at most 2 in flight)

  // warm path (IBFT_FLAG_PUBKEY_CACHE): recovered keys + per-validator fixed-base tables
  bool cache_on = false;       // flag set AND the device's key cache could be set up for this validator set
  DevBuf d_warm_done;
  std::vector<uint8_t> valset_addrs;  // last address list, to keep the cache across identical sets
  uint32_t warm_passes = 0, cold_passes = 0, last_group = 0, last_cold_group = 1;
  bool cold_group_auto = true;
  uint32_t cold_group_force = 0;  // IBFT_COLD_LANES=1|2|4|8|64 (experiments: pin the cold kernel variant)
  // IBFT_COLD_TABLE=lds|private|private2 pins where the lane / group cold kernels keep their window tables: 1 LDS, 2 private
  // segment with the prefetch (round 4's form), 3 private segment without it (two resident wavefronts; lane kernel only)
  uint32_t cold_table_force = 0, last_cold_table = 0;
  uint32_t warm_group_force = 0;  // IBFT_WARM_LANES=1|2|…|64 (experiments: pin the warm kernel variant)
  uint32_t rows_kernel_max = 8192;  // AUTO: a DPP row per signature above wave_rows_max up to this many rows
                                    // (4 096 rows: 0.55 ms vs 0.84 ms for the 8-lane kernel; 8 192: 0.84 vs 0.86)
  uint32_t pair_rows_max = 512;   // AUTO: TWO wavefronts per signature up to this many rows (≤ one wavefront per SIMD in all;
                                  // IBFT_PAIR_ROWS_MAX=0 turns the form off)
  uint32_t wave_rows_max = 2048;  // AUTO: one wavefront per signature up to this many rows (two per SIMD: 0.45 ms); the
                                  // row-per-signature kernel (0.55 ms up to 4 096 rows) wins from there
  // AUTO: the row-per-signature kernel with a helper wavefront per four signatures (scalars, u1·G on the same SIMD) up to
  // this many rows — where the plain form runs at most one wavefront per SIMD; IBFT_ROWS_PAIR=0|1 pins either form
  uint32_t rows_pair_max = 4096;
  int rows_pair_force = -1;
  // ... whose helper wavefronts END once they have published u1·G (kernels.hip.h: rows_pair_handover) where the launch covers
  // at least 5/8 of the device's compute units with a workgroup each: the next pipelined pass then finds room beside this
  // one's main wavefronts two thirds of a pass sooner.  A smaller launch leaves the next pass idle compute units enough, and
  // there a helper parked at barrier 2 keeps that pass off this one's SIMDs.  Measured, per step with the helpers gone
  // (profiles/r27_helper_leave_ab.txt): 129 workgroups of 256 compute units + 0.9 %, 160 − 1.5 %, 188 − 0.8 %, 224 − 2.7 %,
  // 256 − 5.9 %.  IBFT_PAIR_LEAVE=0|1 pins it.
  uint32_t compute_units = 0;
  int pair_leave_force = -1;

  // a1: the proposal whose Keccak the device holds in d_H (raw ‖ BE64(round)); the same proposal is checked
  // against every PREPARE and COMMIT set of a round and on every wake-up, so it is hashed once
  std::vector<uint8_t> hashed_proposal;
  std::vector<uint8_t> padded_proposal;  // the same with Keccak's pad10*1, as uploaded
  bool have_H = false;
  // the proposal is hashed on a stream of its own (one lane, ≈9 µs per 136-byte block): a message set's verdict launch does
  // not depend on it — only the combine step inside the tally does — so the two overlap
  hipStream_t hstream = nullptr;
  hipEvent_t ev_H = nullptr;
  bool H_pending = false;  // the main stream has not yet been told to wait for ev_H
  // Where the proposal is hashed: on the host by default (IBFT_PROPOSAL_HASH=device selects the wavefront sponge kernel)
  bool hash_on_host = true;
  bool H_copy_issued = false;   // ev_H marks a copy out of the pinned staging slot
  uint8_t H_host[32] = {0};     // the digest d_H holds, when the host computed it
  bool have_H_host = false;

  // staged batch
  uint32_t staged_n = 0;
  bool staged_pre = false;

  // pinned host mirrors for results
  uint64_t *h_mask = nullptr;
  uint64_t *h_tally = nullptr;
  uint64_t *h_digest = nullptr;  // 32-byte staging for a1 digests (never shared with results a kernel may still deliver)
  uint64_t *dh_mask = nullptr, *dh_tally = nullptr;  // the same pinned buffers as the device sees them
  // message sets (ibft_verify_messages): sender words then valid words, ⌈max_rows/64⌉ each
  uint64_t *h_set = nullptr, *dh_set = nullptr;
  DevBuf d_set;
  uint8_t *h_class = nullptr, *dh_class = nullptr;  // one routing byte per wire row (ibft_verify_messages_wire)
  DevBuf d_class;
  CertState cert;  // certificates from wire bytes (ibft_verify_certificates_wire, ibft_judge_certificates_wire)
  bool gather_pinned = true;  // columns in ibft_pinned_alloc buffers are read by one gather launch (IBFT_NO_GATHER=1: never)
  // … whose extra blocks can hash PayloadNoSig straight from the host column (IBFT_DIGEST_FUSION=1).  Off by default: it
  // saves nothing measurable (gather + digest ≈ 46 µs either way) and the 8 192-row known-key kernel of a COMMIT set ran
  // 0.25 ms instead of 0.17 ms behind the variant of the launch that carries the digest blocks' 32 KiB of LDS
  // (profiles/r02q_n4096_seq_kernel_stats.csv against r02r)
  bool digest_in_gather = false;
  uint32_t gathers = 0;       // batches whose columns came in through the gather launch
  bool host_direct = false;                          // the last tally kernel delivered its results there
  hipEvent_t ev_ready = nullptr, ev_read = nullptr;  // ibft_seals_export_on: results ready / results read
  bool read_pending = false;                         // the next tally must wait for ev_read

  // dominant-kernel timing
  uint32_t time_every = 1;     // HIP-event pair around the verdict kernels of every n-th staged pass (0 = never)
  uint32_t pass_counter = 0;
  std::vector<hipEvent_t> ev;  // pairs
  uint32_t ev_used = 0;
};

namespace {

#define HIPCHK(ctx, expr)                                                        \
  do {                                                                           \
    hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess) {                                                      \
      (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(e_);     \
      return IBFT_E_HIP;                                                         \
    }                                                                            \
  } while (0)

int ensure(ibft_ctx *c, DevBuf &b, size_t bytes) {
  if (bytes <= b.cap) return IBFT_OK;
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  size_t want = bytes < 256 ? 256 : bytes;
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess) {
    c->last_error = std::string("hipMalloc: ") + hipGetErrorString(e);
    return IBFT_E_NOMEM;
  }
  b.cap = want;
  return IBFT_OK;
}

// The same for a page-locked host array of `elem`-byte entries (at least 256 of them); nothing may still write the old one.
int grow_pinned(void **p, size_t *cap, size_t want, size_t elem) {
  if (want <= *cap) return IBFT_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t n = std::max<size_t>(want, 256);
  if (hipHostMalloc(p, n * elem) != hipSuccess) {
    *p = nullptr;
    return IBFT_E_NOMEM;
  }
  *cap = n;
  return IBFT_OK;
}

int mask_words(size_t n) { return (int)((n + 63) / 64); }

int alloc_rows(ibft_ctx *c, uint32_t rows) {
  size_t m = rows;
  int rc;
  const void *old_mask = c->d_mask.p;
  if ((rc = ensure(c, c->d_hash, m * 32))) return rc;
  if ((rc = ensure(c, c->d_sig, m * 65 + 64))) return rc;
  if ((rc = ensure(c, c->d_signer, m * 20))) return rc;
  if ((rc = ensure(c, c->d_signer_out, m * 20))) return rc;
  if ((rc = ensure(c, c->d_pre, m))) return rc;
  if ((rc = ensure(c, c->d_hash_len, m))) return rc;
  if ((rc = ensure(c, c->d_off, (m + 1) * 4))) return rc;
  if ((rc = ensure(c, c->d_mask, (size_t)mask_words(m) * 8))) return rc;
  if ((rc = ensure(c, c->d_mask_out, (size_t)mask_words(m) * 8))) return rc;
  // fresh memory — or words beyond the rows the last clean covered (a small context's mask buffer is never smaller
  // than 256 bytes, so growing row_cap need not reallocate it): the next verdict launch zeroes the whole mask first
  if (c->d_mask.p != old_mask || rows > c->row_cap) c->mask_dirty_words = ~0u;
  if ((rc = ensure(c, c->d_vidx, m * 4))) return rc;
  {  // the pair a side-stream tally works on (ibft_seals_submit): same sizes, same rule for fresh words
    const void *old_b = c->d_mask_b.p;
    if ((rc = ensure(c, c->d_mask_b, (size_t)mask_words(m) * 8))) return rc;
    if (c->d_mask_b.p != old_b || rows > c->row_cap) c->mask_dirty_words_b = ~0u;
    if ((rc = ensure(c, c->d_vidx_b, m * 4))) return rc;
  }
  if ((rc = ensure(c, c->d_tally, (size_t)ibftk::TALLY_OUT_WORDS * 8))) return rc;
  if ((rc = ensure(c, c->d_acc, (size_t)ibftk::TALLY_ACC_WORDS * 8))) return rc;
  if ((rc = ensure(c, c->d_quorum, (size_t)ibftk::TALLY_SUM_WORDS * 8))) return rc;
  if ((rc = ensure(c, c->d_H, 4 * 8))) return rc;
  if ((rc = ensure(c, c->d_warm_done, m))) return rc;
  c->row_cap = std::max(c->row_cap, rows);
  return IBFT_OK;
}

// row_base (a multiple of 64): the batch is rows [row_base, row_base + n) of the columns — its own verdict words
ibftk::recover_args make_args(ibft_ctx *c, uint32_t n, bool with_pre, uint32_t row_base = 0) {
  ibftk::recover_args a{};
  a.hash32 = (const uint8_t *)c->d_hash.p + 32ull * row_base;
  a.sig65 = (const uint8_t *)c->d_sig.p + 65ull * row_base;
  a.signer20 = (const uint8_t *)c->d_signer.p + 20ull * row_base;
  a.pre_flags = with_pre ? (const uint8_t *)c->d_pre.p + row_base : nullptr;
  a.payload = (const uint8_t *)c->d_payload.p;
  a.off = (const uint32_t *)c->d_off.p + row_base;  // (the offsets themselves are absolute positions in `payload`)
  a.gtab = (const uint32_t *)c->dev->d_gtab.p;
  a.vtab = (const uint32_t *)c->d_vtab.p;
  a.vslot_mask = c->vslot_mask;
  a.n = n;
  a.flags = c->flags;
  a.mask = (uint64_t *)c->d_mask.p + row_base / 64;
  a.vidx = (int32_t *)c->d_vidx.p + row_base;
  a.signer_out = (uint8_t *)c->d_signer_out.p + 20ull * row_base;
  if (c->cache_on) {  // (the caller holds c->dev->mu: the pointers cannot move before the launch is enqueued)
    a.pub = (uint32_t *)c->dev->d_pub.p;
    a.pub_state = (uint32_t *)c->dev->d_state.p;
    a.learned = (uint32_t *)c->dev->d_learned.p;
    a.qtab = (const uint32_t *)c->dev->d_qtab.p;
    a.dummy_validator = c->dev->dummy_slot;
    a.vslot = (const uint32_t *)c->d_vslot.p;
  }
  return a;
}

int next_events(ibft_ctx *c, hipEvent_t *start, hipEvent_t *stop) {
  if ((size_t)c->ev_used * 2 + 2 > c->ev.size()) {
    hipEvent_t a, b;
    HIPCHK(c, hipEventCreate(&a));
    HIPCHK(c, hipEventCreate(&b));
    c->ev.push_back(a);
    c->ev.push_back(b);
  }
  *start = c->ev[(size_t)c->ev_used * 2];
  *stop = c->ev[(size_t)c->ev_used * 2 + 1];
  c->ev_used++;
  return IBFT_OK;
}
// Is the verdict launch about to be enqueued one of the timed ones (every time_every-th)?  Event pairs accumulate until
// ibft_last_kernel_ms reads (and resets) them; unread, they are reused from the first one on.
bool next_pass_timed(ibft_ctx *c) {
  if (c->ev_used >= 4096) c->ev_used = 0;
  return c->time_every && (c->pass_counter++ % c->time_every) == 0;
}

// The segmented tally's records (4 words per block) → the caller's ibft_tally_t; quorum_of_block(b): the two low quorum
// words block b was judged under.  No rows at all: every block is empty, power 0 < quorum.
template <class Q>
void fill_block_tallies(ibft_tally_t *out_tally, uint32_t nb, uint32_t nr, const uint64_t *records, Q quorum_of_block) {
  if (!out_tally) return;
  for (uint32_t b = 0; b < nb; b++) {
    ibft_tally_t &t = out_tally[b];
    memset(&t, 0, sizeof t);
    const uint64_t *q = quorum_of_block(b);
    t.quorum_lo = q[0];
    t.quorum_hi = q[1];
    if (!nr) continue;
    const uint64_t *r = records + 4ull * b;
    t.power_lo = r[0];
    t.power_hi = r[1];
    t.valid_rows = (uint32_t)(r[2] & 0xFFFFFFFFull);
    t.distinct_senders = (uint32_t)(r[2] >> 32);
    t.has_quorum = (uint32_t)r[3];
  }
}

// zero the work mask unless the last tally already left it zero
int clean_mask(ibft_ctx *c, hipStream_t vs) {
  if (c->mask_dirty_words == 0) return IBFT_OK;
  HIPCHK(c, hipMemsetAsync(c->d_mask.p, 0, (size_t)mask_words(c->row_cap) * 8, vs));
  c->mask_dirty_words = 0;
  return IBFT_OK;
}

// Host-side drain of what the pipeline put beside the main stream: the tally stream and the second verdict stream.
void drain_pipeline_streams(ibft_ctx *c) {
  if (c->alt_used) (void)hipStreamSynchronize(c->hstream);
  if (c->tstream) (void)hipStreamSynchronize(c->tstream);
}
// The main stream behind every tally the pipeline put on the side stream, and with it behind every verdict launch the
// pipeline put on the second verdict stream — each pass's tally follows its verdict launch, and ev_pass follows the tally
// (a device-side wait; nothing when none is pending).
int join_side(ibft_ctx *c) {
  if (!c->side_pending) return IBFT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  for (int i = 0; i < 2; i++)
    if (c->ev_pass[i] && hipStreamWaitEvent(c->stream, c->ev_pass[i], 0) != hipSuccess) drain_pipeline_streams(c);
  c->side_pending = false;
  return IBFT_OK;
}
// The lock every entry point takes — and, for all but the pipeline's own calls (ibft_seals_submit / _collect / _stage_next /
// _swap / _rows, the timing getters), the join above: whatever the call enqueues on the main stream finds the buffers a side
// tally works on (work mask, validator indices, tally sums, verdict words) finished with.
struct ctx_lock {
  std::lock_guard<std::mutex> g;
  explicit ctx_lock(ibft_ctx *c) : g(c->mu) {
    c->main_touched = true;
    if (c->side_pending && join_side(c) != IBFT_OK) {  // (cannot report from here: drain the side streams the hard way)
      drain_pipeline_streams(c);
      c->side_pending = false;
    }
  }
};

// While one lives (c->mu held), "the validator set" of the context — table, slot mask, size, key-cache slots and their
// counters — is the family's union, and the context's own set waits in the family's fields; the destructor puts both back.
// EXCHANGED (what make_args, enqueue_recover, recount_built, build_new_tables and key_cache_map / _unmap read): d_vtab, d_vslot,
// vslot, vslot_mask, n_validators, my_built, seen_build_epoch, cache_on.  A field added to the context that these helpers read
// as part of "the validator set" belongs in exchange().
// NOT exchanged — they stay the SINGLE set's while a view lives, and nothing on the _sets path may read them: have_valset,
// d_vpower, d_quorum, quorum_w, power_words, d_seen, h_vtab, valset_addrs, height, last_wide.  Their family counterparts are
// read from c->fam directly (enqueue_block_tally: fam.d_power, d_quorum, power_words, d_seen, largest_set;
// check_block_batch_locked: fam.have, fam.n_sets; block_seals_impl / the submit: fam.quorum).
struct family_view {
  ibft_ctx *c;
  static void exchange(ibft_ctx *c) {
    ValFamily &f = c->fam;
    std::swap(c->d_vtab, f.d_vtab);
    std::swap(c->d_vslot, f.d_vslot);
    c->vslot.swap(f.vslot);
    std::swap(c->vslot_mask, f.vslot_mask);
    std::swap(c->n_validators, f.n_union);
    std::swap(c->my_built, f.my_built);
    std::swap(c->seen_build_epoch, f.seen_build_epoch);
    std::swap(c->cache_on, f.cache_on);
  }
  bool on;
  explicit family_view(ibft_ctx *cc, bool on_ = true) : c(cc), on(on_) {
    if (on) exchange(c);
  }
  ~family_view() {
    if (on) exchange(c);
  }
  family_view(const family_view &) = delete;
  family_view &operator=(const family_view &) = delete;
};

// enqueue the verdict kernels over the resident columns: warm kernel first when tables exist
// (its rows are then skipped by the recover kernel), recover kernel for everything else
// mode: ibftk::MODE_SEALS / MODE_SENDERS, or MODE_EMIT (ibft_recover_seals: bare seals, the recovered address goes to
// d_signer_out) — always the cold branch, no warm stage in front even when tables are built: a warm kernel needs a claimed key to
// pick a table.  Thresholds, pins and the split are those of the other modes.
// keep_mask: a second batch of the same call (rows [row_base, row_base + n)): the work mask already holds the first batch's
// bits and must not be zeroed again (the caller saw to it that this batch's words are clean)
// validators of this context's set whose table is built, recounted when a build pass has run since the last count
void recount_built(ibft_ctx *c) {  // c->dev->mu held
  if (!c->cache_on || c->seen_build_epoch == c->dev->build_epoch) return;
  uint32_t k = 0;
  for (uint32_t sl : c->vslot) k += (sl != 0xFFFFFFFFu && c->dev->built[sl]) ? 1u : 0u;
  c->my_built = k;
  c->seen_build_epoch = c->dev->build_epoch;
}

// A runtime choice — the mode, the lanes per signature, where a table lives — as the template argument of a kernel:
// f(std::integral_constant<int, V>{}) for the V of the list that equals v, for the LAST of the list when none does.
template <int V, int... Rest, class F>
void with_int(int v, F &&f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>{});
  else if (v == V) f(std::integral_constant<int, V>{});
  else with_int<Rest...>(v, f);
}
template <class F>
void with_cold_mode(int mode, F &&f) { with_int<ibftk::MODE_SEALS, ibftk::MODE_EMIT, ibftk::MODE_SENDERS>(mode, f); }
template <class F>
void with_warm_mode(int mode, F &&f) { with_int<ibftk::MODE_SEALS, ibftk::MODE_SENDERS>(mode, f); }  // (the verify kernels know no MODE_EMIT)
template <class F>
void with_qtab_form(int form, F &&f) { with_int<ibftk::QTAB_GLV, ibftk::QTAB_WIDE>(form, f); }
template <class F>
void with_power_words(uint32_t pw, F &&f) { with_int<1, 4>((int)pw, f); }  // PW of the tally kernels: u64 powers, else 256-bit

// ---- the host side of every tally launch -----------------------------------------------------------------------------------------
// A consumer stream may still be copying the previous results (ibft_seals_export_on / exchange): the tally that overwrites
// them waits for it.
static int wait_for_readers(ibft_ctx *c, hipStream_t stream) {
  if (c->read_pending) {
    HIPCHK(c, hipStreamWaitEvent(stream, c->ev_read, 0));
    c->read_pending = false;
  }
  return IBFT_OK;
}
// A tally (and the kernels that finish its work: the seal combine) zeroes exactly the words of the work mask it walked —
// [0, words).  The mask is clean only if no earlier call left bits BEYOND them: mask_dirty_words goes to 0 when the walk covered
// every word that may hold bits, and stays what it was otherwise.  (One copy of this rule once compared against the wrong
// count, and stale bits beyond row 65 536 were accepted as verdicts.)
static void mask_consumed(ibft_ctx *c, size_t words) {
  if ((uint32_t)words >= c->mask_dirty_words) c->mask_dirty_words = 0;
}
// The distinct-sender bitmap of a tally kernel — one bit per entry — lives in dynamic LDS while it fits
// ibftk::TALLY_BITMAP_LDS_MAX (393 216 entries); beyond, the kernel sets every row's bit in the HBM bitmap directly.
// Returns the kernel's lds_bitmap flag, *dyn_bytes: the launch's dynamic LDS size.
static uint32_t bitmap_in_lds(size_t entries, size_t *dyn_bytes) {
  const size_t bytes = (entries + 31) / 32 * 4;
  const bool fits = bytes <= ibftk::TALLY_BITMAP_LDS_MAX;
  *dyn_bytes = fits ? bytes : 0;
  return fits ? 1u : 0u;
}

// one verdict kernel over `items` rows (or wavefronts), per_block of them in a workgroup of `threads`
template <class K>
void launch_verdict(hipStream_t vs, const ibftk::recover_args &a, K kernel, uint32_t items, uint32_t per_block, uint32_t threads) {
  hipLaunchKernelGGL(kernel, dim3((items + per_block - 1) / per_block), dim3(threads), 0, vs, a);
}

// the warm kernel with G lanes per signature: 1 the LDS-staged lane kernel, 64 one wavefront per signature, groups between
// form: the pool's table form (DeviceShared::form) — every width exists in both
void launch_warm(hipStream_t vs, const ibftk::recover_args &a, uint32_t n, int mode, uint32_t G, int form) {
  with_warm_mode(mode, [&](auto M) {
    with_qtab_form(form, [&](auto F) {
      constexpr int MODE = decltype(M)::value, FORM = decltype(F)::value;
      if (G == 1)
        launch_verdict(vs, a, ibftk::verify_known_lane_kernel<MODE, FORM>, n, ibftk::ROWS_PER_BLOCK, ibftk::ROWS_PER_BLOCK);
      else if (G == 64)
        launch_verdict(vs, a, ibftk::verify_known_wave_kernel<MODE, FORM>, n, ibftk::WAVE_KERNEL_WAVES, 64 * ibftk::WAVE_KERNEL_WAVES);
      else
        with_int<32, 16, 8, 4, 2>((int)G, [&](auto GG) {
          constexpr int LANES = decltype(GG)::value;
          launch_verdict(vs, a, ibftk::verify_known_group_kernel<MODE, LANES, FORM>, n, 64 / LANES, 64);
        });
    });
  });
}

// lanes per signature of the cold kernel a batch of n rows gets (what launch_cold takes): pinned, or by the batch's size
uint32_t cold_lanes_for(const ibft_ctx *c, uint32_t n) {
  if (c->cold_group_force) return c->cold_group_force;
  if (!c->cold_group_auto) return 1;
  if ((uint64_t)n <= c->pair_rows_max) return 128;
  if ((uint64_t)n <= c->wave_rows_max) return 64;
  if ((uint64_t)n <= c->rows_kernel_max) return 16;
  if ((uint64_t)n * 8 <= 65536ull) return 8;
  if ((uint64_t)n * 4 <= 65536ull) return 4;
  if ((uint64_t)n * 2 <= 65536ull) return 2;
  return 1;
}
// ... and, of the row forms (16 lanes), the one with a helper wavefront per four signatures
bool rows_pair_for(const ibft_ctx *c, uint32_t n) { return c->rows_pair_force >= 0 ? c->rows_pair_force != 0 : (uint64_t)n <= c->rows_pair_max; }

// the cold kernel with CG lanes per signature: 128 two wavefronts, 64 one, 16 the row forms (four signatures per wavefront, with
// or without a helper wavefront), 8 / 4 / 2 lane groups, 1 the LDS-staged lane kernel; sets what ibft_last_cold_table reports
void launch_cold(ibft_ctx *c, hipStream_t vs, const ibftk::recover_args &a, uint32_t n, int mode, uint32_t CG) {
  with_cold_mode(mode, [&](auto M) {
    constexpr int MODE = decltype(M)::value;
    if (CG == 128) {
      launch_verdict(vs, a, ibftk::ecrecover_wave2_kernel<MODE>, n, ibftk::PAIRS_PER_BLOCK, 128 * ibftk::PAIRS_PER_BLOCK);
    } else if (CG == 64) {
      launch_verdict(vs, a, ibftk::ecrecover_wave_kernel<MODE>, n, ibftk::WAVE_KERNEL_WAVES, 64 * ibftk::WAVE_KERNEL_WAVES);
    } else if (CG == 16) {
      const uint32_t waves = (n + 3) / 4;
      if (rows_pair_for(c, n)) {
        const uint32_t blocks = (waves + ibftk::ROWS_PAIRS_PER_BLOCK - 1) / ibftk::ROWS_PAIRS_PER_BLOCK;
        const bool leave = c->pair_leave_force >= 0 ? c->pair_leave_force != 0 : (uint64_t)blocks * 8 >= (uint64_t)c->compute_units * 5;
        if (leave)
          launch_verdict(vs, a, ibftk::ecrecover_rows_pair_kernel<MODE, false>, waves, ibftk::ROWS_PAIRS_PER_BLOCK, 128 * ibftk::ROWS_PAIRS_PER_BLOCK);
        else
          launch_verdict(vs, a, ibftk::ecrecover_rows_pair_kernel<MODE, true>, waves, ibftk::ROWS_PAIRS_PER_BLOCK, 128 * ibftk::ROWS_PAIRS_PER_BLOCK);
      } else
        launch_verdict(vs, a, ibftk::ecrecover_rows_kernel<MODE>, waves, ibftk::WAVE_KERNEL_WAVES, 64 * ibftk::WAVE_KERNEL_WAVES);
    } else if (CG > 1) {
      // the lanes' window tables: LDS (no private segment) unless pinned otherwise (IBFT_COLD_TABLE=private: round 4's form, A/B)
      const bool lds_tab = c->cold_table_force != 2;
      with_int<8, 4, 2>((int)CG, [&](auto GG) {
        with_int<ibftk::TAB_LDS, ibftk::TAB_PRIVATE_PREFETCH>(lds_tab ? ibftk::TAB_LDS : ibftk::TAB_PRIVATE_PREFETCH, [&](auto TT) {
          constexpr int LANES = decltype(GG)::value, TAB = decltype(TT)::value;
          launch_verdict(vs, a, ibftk::ecrecover_group_kernel<MODE, LANES, TAB>, n, 64 / LANES, 64);
        });
      });
      c->last_cold_table = lds_tab ? 1 : 2;
    } else {
      // one lane per signature: up to one wavefront per SIMD offered (n ≤ 65 536) the table lives in LDS; beyond, in the private
      // segment WITHOUT the prefetch — 256 registers, two resident wavefronts per SIMD (15 against 18 ns per verify)
      const uint32_t tab = c->cold_table_force ? c->cold_table_force : ((uint64_t)n <= 65536ull ? 1u : 3u);
      with_int<ibftk::TAB_LDS, ibftk::TAB_PRIVATE_PREFETCH, ibftk::TAB_PRIVATE>(
          tab == 1 ? ibftk::TAB_LDS : tab == 2 ? ibftk::TAB_PRIVATE_PREFETCH : ibftk::TAB_PRIVATE, [&](auto TT) {
            launch_verdict(vs, a, ibftk::ecrecover_lane_kernel<MODE, decltype(TT)::value>, n, ibftk::ROWS_PER_BLOCK, ibftk::ROWS_PER_BLOCK);
          });
      c->last_cold_table = tab;
    }
  });
}

// Batches just beyond what one wavefront per SIMD can take (65 536 rows through the lane kernel with its tables in LDS): the
// private-segment form that serves everything larger keeps TWO wavefronts on as many SIMDs as there are rows beyond 65 536 — and
// the launch lasts as long as those: 1.72 ms for 70 000 rows where 65 536 take 0.92 (profiles/r06j_kernel_ab.txt).  Up to
// SPLIT_ROWS_MAX rows the batch is two launches instead — 65 536 rows through the LDS-table lane kernel, the rest through whatever
// the AUTO rule picks for that many rows (rows 65 536 … n are a batch of their own: every kernel takes a row base): 0.92 + 0.33 ms at
// 70 000 rows, 0.92 + 0.75 at 98 304; beyond that the private-segment form wins again (131 072: 1.76 ms).  Cold contexts without
// pinned kernels only (round 6).
constexpr uint32_t SPLIT_ROWS_MIN = 65536u, SPLIT_ROWS_MAX = 98304u;

int enqueue_recover(ibft_ctx *c, hipStream_t vs, uint32_t n, bool with_pre, int mode, bool time_it, uint32_t row_base = 0,
                    bool keep_mask = false, hipEvent_t *stop_out = nullptr) {
  if (stop_out) *stop_out = nullptr;
  if (n == 0) return IBFT_OK;
  if (n > SPLIT_ROWS_MIN && n <= SPLIT_ROWS_MAX && !c->cache_on && c->cold_group_auto && !c->cold_group_force && !c->cold_table_force &&
      row_base % 64 == 0 && c->split_large) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (time_it) {
      int rc = next_events(c, &e0, &e1);
      if (rc) return rc;
      HIPCHK(c, hipEventRecord(e0, vs));
    }
    // The work mask is cleared HERE, once, for both launches: the lane kernel of the first part stores whole verdict words and
    // never asks for a clean mask, the kernel of the second part ORs its bits into words it expects to be zero (a dirty or
    // freshly allocated mask gave wrong verdicts in the rows beyond 65 536: caught by the Byzantine parity test, not by the
    // all-valid A/B rounds).
    int rc = keep_mask ? (int)IBFT_OK : clean_mask(c, vs);
    if (rc) return rc;
    if ((rc = enqueue_recover(c, vs, SPLIT_ROWS_MIN, with_pre, mode, false, row_base, true))) return rc;
    if ((rc = enqueue_recover(c, vs, n - SPLIT_ROWS_MIN, with_pre, mode, false, row_base + SPLIT_ROWS_MIN, true))) return rc;
    if (time_it) {
      HIPCHK(c, hipEventRecord(e1, vs));
      if (stop_out) *stop_out = e1;
    }
    c->last_cold_group = 1;   // (what ibft_last_dispatch reports for a split batch: the lane kernel took the bulk)
    c->last_cold_table = 1;
    c->split_launches++;
    return IBFT_OK;
  }
  std::unique_lock<std::mutex> dev_lk(c->dev->mu, std::defer_lock);
  if (c->cache_on) {
    dev_lk.lock();
    recount_built(c);
  }
  ibftk::recover_args a = make_args(c, n, with_pre, row_base);
  struct dirty_on_exit {  // whatever is launched below writes verdict bits into the first ⌈n/64⌉ words of d_mask
    ibft_ctx *c;
    uint32_t words;
    ~dirty_on_exit() { c->mask_dirty_words = std::max(c->mask_dirty_words, words); }
  } mark_dirty{c, (uint32_t)mask_words((size_t)row_base + n)};
  auto clean_mask = [keep_mask, vs](ibft_ctx *cc) { return keep_mask ? (int)IBFT_OK : ::clean_mask(cc, vs); };
  int rc_clean = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (time_it) {
    int rc = next_events(c, &e0, &e1);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(e0, vs));
  }
  const bool warm = c->cache_on && c->my_built > 0 && mode != ibftk::MODE_EMIT;
  if (warm) {
    a.warm_done = (uint8_t *)c->d_warm_done.p + row_base;
    // lanes per signature: ≈ one wavefront per SIMD (1024 SIMDs × 64 lanes / n rows), a power of two
    uint32_t G = 1;
    if (c->warm_group_force) {
      G = c->warm_group_force;
    } else if (c->kernel == IBFT_KERNEL_WAVE) {
      G = 64;
    } else if (c->kernel != IBFT_KERNEL_LANE) {
      while (G < 64 && (uint64_t)n * (G * 2) <= 65536ull) G *= 2;
    }
    if (G > 1 && (rc_clean = clean_mask(c))) return rc_clean;  // (the lane kernel stores whole verdict words)
    launch_warm(vs, a, n, mode, G, c->dev->form);
    c->last_group = G;
    HIPCHK(c, hipGetLastError());
    c->warm_passes++;
  } else {
    c->cold_passes++;
  }
  if (warm && c->my_built >= c->n_validators) {
    // every validator has a table: the warm kernel decides every row (non-members included)
    if (time_it) {
      HIPCHK(c, hipEventRecord(e1, vs));
      if (stop_out) *stop_out = e1;
    }
    c->last_cold_group = 0;
    return IBFT_OK;
  }
  // cold kernel: lane groups when the batch is too small to fill the chip
  const uint32_t CG = cold_lanes_for(c, n);
  // every form but the lane kernel ORs its bits into the mask: clean unless a warm kernel in front has already cleaned and
  // written it (the lane kernel merges the bits of decided rows into its whole words instead)
  if (CG > 1 && !warm && (rc_clean = clean_mask(c))) return rc_clean;
  launch_cold(c, vs, a, n, mode, CG);
  c->last_cold_group = CG;
  HIPCHK(c, hipGetLastError());
  if (time_it) {
    HIPCHK(c, hipEventRecord(e1, vs));
    if (stop_out) *stop_out = e1;
  }
  return IBFT_OK;
}

// after a fetch: build tables for keys learned since the last build (stream-ordered, asynchronous)
// Keys were learned since the last build pass (the device counter moved): tables for them, on this context's stream.
// One context builds; the others see the new tables at their next launch (state 2) and recount.
int build_new_tables(ibft_ctx *c, uint32_t learned_total, uint32_t any_slot) {
  if (!c->cache_on) return IBFT_OK;
  DeviceShared &d = *c->dev;
  std::lock_guard<std::mutex> lk(d.mu);
  if ((int32_t)(learned_total - d.learned_seen) <= 0) {  // (another context's pass may already have covered a newer count)
    recount_built(c);
    return IBFT_OK;
  }
  const uint32_t ns = d.used;
  hipLaunchKernelGGL(ibftk::qtab_claim_kernel, dim3((ns + 255) / 256), dim3(256), 0, c->stream, (uint32_t *)d.d_state.p, ns);
  HIPCHK(c, hipGetLastError());
  with_qtab_form(d.form, [&](auto F) {
    constexpr int FORM = decltype(F)::value;
    constexpr uint32_t WINDOWS = FORM == ibftk::QTAB_GLV ? ibftk::QGLV_WINDOWS : ibftk::QTAB_WINDOWS;
    hipLaunchKernelGGL(ibftk::qtab_build_kernel<FORM>, dim3(((ns + 63) / 64) * WINDOWS), dim3(64), 0, c->stream,
                       (const uint32_t *)d.d_pub.p, (const uint32_t *)d.d_state.p, (uint32_t *)d.d_qtab.p, ns);
  });
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(ibftk::qtab_commit_kernel, dim3((ns + 255) / 256), dim3(256), 0, c->stream, (uint32_t *)d.d_state.p, ns);
  HIPCHK(c, hipGetLastError());
  // which slots hold a table now: the host's shadow of the states (a learn event is rare once the set is known)
  std::vector<uint32_t> st(ns);
  HIPCHK(c, hipMemcpyAsync(st.data(), d.d_state.p, (size_t)ns * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (uint32_t i = 0; i < ns; i++) d.built[i] = st[i] == ibftk::KEY_BUILT;
  d.learned_seen = learned_total;
  if (any_slot < ns && d.built[any_slot]) d.dummy_slot = any_slot;
  d.build_epoch++;
  recount_built(c);
  return IBFT_OK;
}

// `on`: the stream the tally is enqueued on (default: the context's main stream; ibft_seals_submit passes the side stream)
int enqueue_tally(ibft_ctx *c, uint32_t n, const ibftk::set_args *set = nullptr, hipStream_t on = nullptr) {
  const hipStream_t ts = on ? on : c->stream;
  int rc;
  if ((rc = wait_for_readers(c, ts))) return rc;
  ibftk::tally_args t{};
  t.work_mask = (uint64_t *)c->d_mask.p;
  t.mask = (uint64_t *)c->d_mask_out.p;
  t.vidx = (const int32_t *)c->d_vidx.p;
  t.vpower32 = (const uint32_t *)c->d_vpower.p;
  t.n = n;
  t.n_validators = c->n_validators;
  t.seen = (uint32_t *)c->d_seen.p;
  t.acc = (uint64_t *)c->d_acc.p;
  t.quorum = (const uint64_t *)c->d_quorum.p;
  t.out = (uint64_t *)c->d_tally.p;
  t.host_mask = c->tally_slot >= 0 ? c->dp_mask[c->tally_slot] : c->dh_mask;
  t.host_tally = c->tally_slot >= 0 ? c->dp_tally[c->tally_slot] : c->dh_tally;
  t.set_on = set ? 1u : 0u;
  if (set) t.set = *set;
  // HasPrepareQuorum: on one device the proposer's seat joins the bitmap here; a rank of a sharded batch only counts the
  // proposer's rows and leaves the seat to the merge (exchange_unpack_kernel)
  t.prop_on = c->next_prop_on ? 1u : 0u;
  t.prop_vidx = c->next_prop_vidx;
  t.prop_seat = c->next_shard ? 0u : 1u;
  c->next_prop_on = false;
  c->next_prop_vidx = -1;
  c->next_shard = false;
  if (c->cache_on) t.learned_src = (const uint64_t *)c->dev->d_learned.p;
  if (c->comm || c->xlocal) {  // a rank of a sharded batch: the bitmap of this launch is what the exchange merges
    const size_t bytes = (size_t)((c->n_validators + 63) / 64) * 8;
    if (bytes > c->d_seen_out.cap) {
      if ((rc = ensure(c, c->d_seen_out, bytes))) return rc;
      HIPCHK(c, hipMemsetAsync(c->d_seen_out.p, 0, c->d_seen_out.cap, ts));  // (an odd trailing 32-bit word stays 0)
    }
    t.seen_out = (uint32_t *)c->d_seen_out.p;
  }
  const dim3 grid(std::max(1u, (n + ibftk::TALLY_ROWS_PER_BLOCK - 1) / ibftk::TALLY_ROWS_PER_BLOCK)), block(ibftk::TALLY_THREADS);
  // one workgroup (n ≤ 4 096): everything stays in the workgroup — no global atomics on the latency-critical sizes;
  // beyond: ticket form, each workgroup merging its LDS bitmap into the HBM one word by word.  A validator set whose
  // bitmap does not fit 48 KiB of dynamic LDS (> 393 216 validators) sends every row's bit to HBM directly.
  size_t dyn;
  t.lds_bitmap = bitmap_in_lds(c->n_validators, &dyn);
  // (a side-stream tally has to FIT next to a resident verdict kernel: the one-workgroup form holds 126 registers in each of its
  // sixteen wavefronts — nothing else fits a compute unit beside it —, the ticket form 42)
  const bool single = grid.x == 1 && t.lds_bitmap && !on;
  with_power_words(c->power_words, [&](auto PW) {
    if (single) hipLaunchKernelGGL((ibftk::tally_kernel<decltype(PW)::value, false>), grid, block, dyn, ts, t);
    else hipLaunchKernelGGL((ibftk::tally_kernel<decltype(PW)::value, true>), grid, block, dyn, ts, t);
  });
  HIPCHK(c, hipGetLastError());
  c->host_direct = c->dh_mask != nullptr && c->tally_slot < 0;  // results of THIS tally are on their way to h_mask / h_tally
  mask_consumed(c, mask_words(n));
  return IBFT_OK;
}

int fetch_results(ibft_ctx *c, uint32_t n, uint64_t *out_mask, ibft_tally_t *tally, bool have_tally) {
  size_t mw = (size_t)mask_words(n);
  const bool direct = c->host_direct && have_tally;  // the tally kernel already wrote h_mask / h_tally
  c->host_direct = false;
  if (!direct) {
    if (out_mask && mw)
      HIPCHK(c, hipMemcpyAsync(c->h_mask, have_tally ? c->d_mask_out.p : c->d_mask.p, mw * 8, hipMemcpyDeviceToHost,
                               c->stream));
    // d_tally holds {power_lo, power_hi, counts, has_quorum, learned|any_validator, power in full}: one copy
    if (tally && have_tally)
      HIPCHK(c, hipMemcpyAsync(c->h_tally, c->d_tally.p, (size_t)(ibftk::TALLY_OUT_PROPOSER_ROWS + 1) * 8,
                               hipMemcpyDeviceToHost, c->stream));
    // {keys learned, a learned slot}: the device-wide counter itself (a tally kernel passes it on in word 4 of its results;
    // calls without a tally — the certificate tree, plain hash batches — read it here)
    if (c->cache_on)
      HIPCHK(c, hipMemcpyAsync(c->h_tally + 4, c->dev->d_learned.p, 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->cache_on) {
    const uint32_t *lw = reinterpret_cast<const uint32_t *>(c->h_tally + 4);
    int rcb = build_new_tables(c, lw[0], lw[1]);
    if (rcb) return rcb;
  }
  if (out_mask && mw) {
    memcpy(out_mask, c->h_mask, mw * 8);
    // clear the padding bits of the last word
    if (n & 63) out_mask[mw - 1] &= (~0ull) >> (64 - (n & 63));
  }
  if (have_tally)
    for (int i = 0; i < ibftk::TALLY_SUM_WORDS; i++) c->last_wide[i] = c->h_tally[ibftk::TALLY_OUT_WIDE + i];
  if (tally) {
    memset(tally, 0, sizeof *tally);
    tally->quorum_lo = c->quorum_w[0];
    tally->quorum_hi = c->quorum_w[1];
    if (have_tally) {
      tally->power_lo = c->h_tally[0];
      tally->power_hi = c->h_tally[1];
      tally->valid_rows = (uint32_t)(c->h_tally[2] & 0xFFFFFFFFull);
      tally->distinct_senders = (uint32_t)(c->h_tally[2] >> 32);
      tally->has_quorum = (uint32_t)c->h_tally[3];
      tally->proposer_rows = (uint32_t)c->h_tally[ibftk::TALLY_OUT_PROPOSER_ROWS];
    }
  }
  return IBFT_OK;
}

// validator index of an address in the current set (−1: no validator) — the device's open-addressing table, on the host
int32_t host_lookup(const ibft_ctx *c, const uint8_t addr20[20]) {
  if (c->h_vtab.empty()) return -1;
  uint32_t a[5];
  memcpy(a, addr20, 20);
  uint32_t s = ibftk::addr_hash(a) & c->vslot_mask;
  for (uint32_t probe = 0; probe <= c->vslot_mask; probe++) {
    const uint32_t *e = &c->h_vtab[(size_t)s * 6];
    if (e[5] == 0) return -1;
    if (memcmp(e, a, 20) == 0) return (int32_t)e[5] - 1;
    s = (s + 1) & c->vslot_mask;
  }
  return -1;
}
// the next tally this context enqueues is HasPrepareQuorum with this proposer (null: plain HasQuorum)
void note_proposer(ibft_ctx *c, const uint8_t *proposer20, bool shard = false) {
  c->next_prop_on = proposer20 != nullptr;
  c->next_prop_vidx = proposer20 ? host_lookup(c, proposer20) : -1;
  c->next_shard = shard && proposer20 != nullptr;
}

int upload(ibft_ctx *c, DevBuf &b, const void *src, size_t bytes);

// n hashes of a column, in place: carried proposalHash → the digest the seal signs (no-op under the identity convention).
// The hash column's rows, or the blocks' hashes of a synchronous block call before they are spread over their rows.
// keep_copy: the carried hashes stay available in d_hash_copy (rows [0, n)) for the a1 compare
int apply_seal_digest(ibft_ctx *c, void *col, uint32_t n, bool keep_copy = false) {
  if (c->seal_digest_mode == 0 || n == 0) return IBFT_OK;
  ibftk::seal_digest_args a{};
  a.hash32 = (uint8_t *)col;
  if (keep_copy) {
    int rc = ensure(c, c->d_hash_copy, (size_t)n * 32);
    if (rc) return rc;
    a.copy32 = (uint8_t *)c->d_hash_copy.p;
  }
  a.n = n;
  memcpy(a.suffix_words, c->seal_suffix_words, sizeof a.suffix_words);
  hipLaunchKernelGGL(ibftk::seal_digest_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return IBFT_OK;
}

// d_H ← keccak256(raw ‖ BE64(round)) unless it already holds exactly that (enqueued on the context's stream)
// d_H ← keccak256(raw ‖ BE64(round)) unless it already holds exactly that.  Two steps so that a message set can put the
// hash commands BEHIND its verdict launch in host time as well (≈20 µs of runtime calls that would otherwise delay the
// uploads): note_proposal decides and pads, launch_proposal_hash enqueues upload + kernel on the side stream.
// Every reader of d_H is a synchronous call that waits for ev_H first (wait_proposal_hash), so nothing else orders the two streams.
bool note_proposal(ibft_ctx *c, const uint8_t *raw, size_t raw_len, uint64_t round) {
  uint8_t be[8];
  for (int i = 0; i < 8; i++) be[i] = (uint8_t)(round >> (8 * (7 - i)));
  if (c->have_H && c->hashed_proposal.size() == raw_len + 8 && (raw_len == 0 || memcmp(c->hashed_proposal.data(), raw, raw_len) == 0) &&
      memcmp(c->hashed_proposal.data() + raw_len, be, 8) == 0)
    return false;
  c->have_H = false;
  c->hashed_proposal.resize(raw_len + 8);
  if (raw_len) memcpy(c->hashed_proposal.data(), raw, raw_len);
  memcpy(c->hashed_proposal.data() + raw_len, be, 8);
  return true;
}
// Keccak-256 of a ‖ b on the HOST, with the device code's own permutation (keccak_dev.h compiles for both sides).
// Keccak is a sequential sponge: one host core absorbs ≈340–360 MB/s here, ≈600 MB/s on the GPU box's cores (3.6 µs for 1 KiB, ≈3 ms for 1 MiB) where the one
// wavefront that can work on a message absorbs 25 MB/s (profiles/r02_a1_sizes_v2.json: 41 ms for 1 MiB).
// the permutation for a host that has BMI1/BMI2 (andn, rorx: every x86-64 core since 2013): the same code, compiled for them
__attribute__((target("bmi,bmi2"), noinline)) static void f1600_bmi(uint64_t s[25]) { keccak::f1600(s); }
static void f1600_plain(uint64_t s[25]) { keccak::f1600(s); }
static void (*const host_f1600)(uint64_t *) = (__builtin_cpu_supports("bmi") && __builtin_cpu_supports("bmi2")) ? f1600_bmi : f1600_plain;

void host_keccak256(const uint8_t *a, size_t na, const uint8_t *b, size_t nb, uint8_t out32[32]) {
  uint64_t s[25] = {0};
  uint8_t block[136];
  size_t fill = 0;
  auto absorb = [&](const uint8_t *p, size_t n) {
    while (n) {
      if (fill == 0 && n >= 136) {  // whole blocks straight from the source
        for (int i = 0; i < 17; i++) {
          uint64_t w;
          memcpy(&w, p + 8 * i, 8);
          s[i] ^= w;
        }
        host_f1600(s);
        p += 136;
        n -= 136;
        continue;
      }
      const size_t k = std::min(n, (size_t)136 - fill);
      memcpy(block + fill, p, k);
      fill += k;
      p += k;
      n -= k;
      if (fill == 136) {
        for (int i = 0; i < 17; i++) {
          uint64_t w;
          memcpy(&w, block + 8 * i, 8);
          s[i] ^= w;
        }
        host_f1600(s);
        fill = 0;
      }
    }
  };
  if (na) absorb(a, na);
  if (nb) absorb(b, nb);
  memset(block + fill, 0, 136 - fill);
  block[fill] ^= 0x01;
  block[135] ^= 0x80;
  for (int i = 0; i < 17; i++) {
    uint64_t w;
    memcpy(&w, block + 8 * i, 8);
    s[i] ^= w;
  }
  host_f1600(s);
  memcpy(out32, s, 32);
}

int launch_proposal_hash(ibft_ctx *c) {
  if (c->hash_on_host) {
    // the digest is computed here, on the calling thread — behind the verdict launch of a message set, which is already
    // running on the device — and reaches d_H through the side stream like the device-computed one did
    if (c->H_copy_issued) HIPCHK(c, hipEventSynchronize(c->ev_H));  // the staging slot is free again
    uint8_t *stage = reinterpret_cast<uint8_t *>(c->h_digest) + 32;
    host_keccak256(c->hashed_proposal.data(), c->hashed_proposal.size(), nullptr, 0, stage);
    memcpy(c->H_host, stage, 32);
    HIPCHK(c, hipMemcpyAsync(c->d_H.p, stage, 32, hipMemcpyHostToDevice, c->hstream));
    HIPCHK(c, hipEventRecord(c->ev_H, c->hstream));
    c->H_copy_issued = true;
    c->H_pending = true;
    c->have_H = true;
    c->have_H_host = true;
    return IBFT_OK;
  }
  c->have_H_host = false;
  // Keccak padding on the host: pad10*1 up to a multiple of the 136-byte rate (the kernel XORs whole 64-bit words)
  const size_t mlen = c->hashed_proposal.size();
  const size_t blocks = mlen / 136 + 1;
  c->padded_proposal.assign(blocks * 136, 0);
  memcpy(c->padded_proposal.data(), c->hashed_proposal.data(), mlen);
  c->padded_proposal[mlen] ^= 0x01;
  c->padded_proposal[blocks * 136 - 1] ^= 0x80;
  int rc = ensure(c, c->d_raw, blocks * 136);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_raw.p, c->padded_proposal.data(), blocks * 136, hipMemcpyHostToDevice, c->hstream));
  hipLaunchKernelGGL(ibftk::proposal_hash_kernel, dim3(1), dim3(64), 0, c->hstream, (const uint64_t *)c->d_raw.p,
                     (uint32_t)blocks, (uint64_t *)c->d_H.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev_H, c->hstream));
  c->H_pending = true;
  c->have_H = true;  // valid once the main stream has waited for ev_H (wait_proposal_hash): every reader does that first
  return IBFT_OK;
}
int ensure_proposal_hash(ibft_ctx *c, const uint8_t *raw, size_t raw_len, uint64_t round) {
  return note_proposal(c, raw, raw_len, round) ? launch_proposal_hash(c) : IBFT_OK;
}
// the main stream goes on only when d_H holds the hash launched by ensure_proposal_hash
int wait_proposal_hash(ibft_ctx *c) {
  if (!c->H_pending) return IBFT_OK;
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_H, 0));
  c->H_pending = false;
  return IBFT_OK;
}

int upload(ibft_ctx *c, DevBuf &b, const void *src, size_t bytes) {
  if (!bytes) return IBFT_OK;
  int rc = ensure(c, b, bytes);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
  return IBFT_OK;
}

// the n + 1 offsets of a batch of byte strings never decrease (off may be null when n == 0)
bool offsets_ok(const uint32_t *off, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return false;
  return true;
}
// … and a batch that has bytes comes with them
bool bytes_ok(const uint32_t *off, size_t n, const void *bytes) { return !(n && off[n] && !bytes); }

// Blocks handed out by ibft_pinned_alloc: a column that lies inside one can be read by the device directly.
struct PinnedRegistry {
  std::mutex mu;
  std::map<uintptr_t, size_t> blocks;
  bool covers(const void *p, size_t bytes) {
    const uintptr_t a = (uintptr_t)p;
    std::lock_guard<std::mutex> lk(mu);
    auto it = blocks.upper_bound(a);
    if (it == blocks.begin()) return false;
    --it;
    return a >= it->first && a + bytes <= it->first + it->second;
  }
};
PinnedRegistry &pinned_registry() {
  static PinnedRegistry r;
  return r;
}

// The host→HBM column copies of one batch.  flush(): ONE gather launch when every source is pinned (the device
// reads the columns itself), otherwise one hipMemcpyAsync per column as before.
struct ColumnCopies {
  struct Seg {
    void *dst;
    const void *src;
    size_t bytes;
  };
  Seg seg[ibftk::GATHER_MAX];
  int n = 0;
  // optional: the PayloadNoSig column of a message set.  Pinned: it is never copied — digest blocks of the gather launch
  // hash it straight from the host column into `digest_dst` (digest_done).  Pageable: payload and offsets are copied to
  // pay_dst / off_dst like any column and the caller launches payload_digest_kernel.
  const void *pay_src = nullptr, *off_src = nullptr;
  void *pay_dst = nullptr, *off_dst = nullptr, *digest_dst = nullptr;
  size_t pay_bytes = 0, rows = 0;
  bool digest_done = false;
  void add(void *dst, const void *src, size_t bytes) {
    if (bytes && n < ibftk::GATHER_MAX) seg[n++] = Seg{dst, src, bytes};
  }
  void payload(void *pdst, const void *psrc, size_t pbytes, void *odst, const void *osrc, size_t n_rows, void *ddst) {
    pay_dst = pdst; pay_src = psrc; pay_bytes = pbytes; off_dst = odst; off_src = osrc; rows = n_rows; digest_dst = ddst;
  }
  int flush(ibft_ctx *c) {
    const bool job = rows != 0;
    if (n == 0 && !job) return IBFT_OK;
    bool pinned = c->gather_pinned;
    for (int i = 0; i < n && pinned; i++) pinned = seg[i].bytes < (1ull << 31) && pinned_registry().covers(seg[i].src, seg[i].bytes);
    if (pinned && job)
      pinned = pay_bytes < (1ull << 31) && pinned_registry().covers(off_src, (rows + 1) * 4) &&
               (pay_bytes == 0 || pinned_registry().covers(pay_src, pay_bytes));
    if (!pinned) {
      if (job) {
        if (pay_bytes) HIPCHK(c, hipMemcpyAsync(pay_dst, pay_src, pay_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(off_dst, off_src, (rows + 1) * 4, hipMemcpyHostToDevice, c->stream));
      }
      for (int i = 0; i < n; i++) HIPCHK(c, hipMemcpyAsync(seg[i].dst, seg[i].src, seg[i].bytes, hipMemcpyHostToDevice, c->stream));
      n = 0;
      return IBFT_OK;
    }
    if (job && !c->digest_in_gather) {  // the payload and its offsets as two more copied columns; the caller hashes from HBM
      if (n + 2 > ibftk::GATHER_MAX) return IBFT_E_INVAL;
      if (pay_bytes) seg[n++] = Seg{pay_dst, pay_src, pay_bytes};
      seg[n++] = Seg{off_dst, off_src, (rows + 1) * 4};
    }
    const bool fused = job && c->digest_in_gather;
    ibftk::gather_args a{};
    uint32_t blocks = 0;
    for (int i = 0; i < n; i++) {
      a.src[i] = (const uint8_t *)seg[i].src;
      a.dst[i] = (uint8_t *)seg[i].dst;
      a.bytes[i] = (uint32_t)seg[i].bytes;
      a.first_block[i] = blocks;
      blocks += (uint32_t)((seg[i].bytes + ibftk::GATHER_BLOCK_BYTES - 1) / ibftk::GATHER_BLOCK_BYTES);
    }
    a.first_block[n] = blocks;
    a.n = (uint32_t)n;
    if (fused) {
      a.pay_src = (const uint8_t *)pay_src;
      a.off_src = (const uint32_t *)off_src;
      a.digest_dst = (uint8_t *)digest_dst;
      a.n_rows = (uint32_t)rows;
      a.pay_bytes = (uint32_t)pay_bytes;
      blocks += (uint32_t)((rows + 63) / 64);
      digest_done = true;
    }
    if (fused)
      hipLaunchKernelGGL(ibftk::gather_columns_kernel<true>, dim3(blocks), dim3(256), 0, c->stream, a);
    else
      hipLaunchKernelGGL(ibftk::gather_columns_kernel<false>, dim3(blocks), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    c->gathers++;
    n = 0;
    return IBFT_OK;
  }
};

// ---- RCCL, loaded on first use: a single-GPU deployment never needs the library ----------------------
struct RcclApi {
  void *handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommCount)(ncclComm_t, int *) = nullptr;
  ncclResult_t (*CommUserRank)(ncclComm_t, int *) = nullptr;
  ncclResult_t (*CommCuDevice)(ncclComm_t, int *) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  bool ok = false;
};
RcclApi *rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    const char *names[] = {getenv("IBFT_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *nm : names) {
      if (!nm || !*nm) continue;
      if ((api.handle = dlopen(nm, RTLD_NOW | RTLD_LOCAL))) break;
    }
    if (!api.handle) return;
#define IBFT_SYM(field, name) api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.handle, name))
    IBFT_SYM(GetUniqueId, "ncclGetUniqueId");
    IBFT_SYM(CommInitRank, "ncclCommInitRank");
    IBFT_SYM(CommDestroy, "ncclCommDestroy");
    IBFT_SYM(AllReduce, "ncclAllReduce");
    IBFT_SYM(CommCount, "ncclCommCount");
    IBFT_SYM(CommUserRank, "ncclCommUserRank");
    IBFT_SYM(CommCuDevice, "ncclCommCuDevice");
    IBFT_SYM(GroupStart, "ncclGroupStart");
    IBFT_SYM(GroupEnd, "ncclGroupEnd");
    IBFT_SYM(GetErrorString, "ncclGetErrorString");
#undef IBFT_SYM
    api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllReduce && api.GroupStart && api.GroupEnd;
  });
  return api.ok ? &api : nullptr;
}
#define NCCLCHK(ctx, api, expr)                                                                              \
  do {                                                                                                       \
    ncclResult_t r_ = (expr);                                                                                \
    if (r_ != ncclSuccess) {                                                                                 \
      (ctx)->last_error = std::string(#expr) + ": " + ((api)->GetErrorString ? (api)->GetErrorString(r_) : "rccl error"); \
      return IBFT_E_RCCL;                                                                                    \
    }                                                                                                        \
  } while (0)

void comm_release(ibft_ctx *c) {
  if (c->comm) {
    if (RcclApi *a = rccl()) (void)a->CommDestroy(c->comm);
    c->comm = nullptr;
  }
  for (int i = 0; i < 2; i++) {
    if (c->ev_xdone[i]) (void)hipEventDestroy(c->ev_xdone[i]);
    c->ev_xdone[i] = nullptr;
    if (c->h_xres[i]) (void)hipHostFree(c->h_xres[i]);
    c->h_xres[i] = c->dh_xres[i] = nullptr;
  }
  c->h_xres_words = 0;
  if (c->ev_xpack) (void)hipEventDestroy(c->ev_xpack);
  c->ev_xpack = nullptr;
  c->xlocal = false;
  if (c->xstream) (void)hipStreamDestroy(c->xstream);
  c->xstream = nullptr;
  c->xrank = 0;
  c->xworld = 1;
  c->x_issued = c->x_fetched = 0;
}

// shard layout (pure): contiguous 64-aligned row ranges, the last rank takes the remainder
uint64_t shard_rows_per_rank(uint64_t n_total, uint32_t world) {
  return (((n_total + world - 1) / world) + 63) / 64 * 64;
}

int ensure_handoff_events(ibft_ctx *c) {
  if (!c->ev_ready) {
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_read, hipEventDisableTiming));
  }
  return IBFT_OK;
}

struct xplan {
  uint32_t slot, w, total_words, seen_words, n_pieces, slots, my_words, K;
  // HasPrepareQuorum of THIS exchange (fixed when the plan is made: a tally some other call enqueues on the context between
  // pack and unpack must not change what the merge applies)
  bool prop_on;
  int32_t prop_vidx;
};
// u64 slots of the exchange buffer: K verdict arrays, one bitmap segment per rank, the count of valid rows
uint32_t exchange_slots(uint32_t K, uint32_t words_per_rank, uint32_t world, uint32_t n_validators) {
  return K * words_per_rank * world + world * ((n_validators + 63) / 64) + 1;
}
// before the collective: order behind the tally, pack this rank's words + its sender bitmap into the exchange buffer.
// n_local rows of this rank (seal batch: the staged one; message set: the last set), K verdict arrays.
int exchange_pre(ibft_ctx *c, uint64_t n_total, xplan &x, uint32_t K = 1, const uint8_t *proposer20 = nullptr) {
  if (!(c->comm || c->xlocal) || !c->have_valset) return (c->comm || c->xlocal) ? IBFT_E_NOVALSET : IBFT_E_INVAL;
  if (c->x_issued - c->x_fetched >= 2) {
    c->last_error = "two exchanges already in flight: call ibft_seals_fetch_merged first";
    return IBFT_E_INVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t per = shard_rows_per_rank(n_total, c->xworld);
  const uint32_t n_local = K == 2 ? c->set_n : c->staged_n;
  x.K = K;
  x.prop_on = proposer20 != nullptr;
  x.prop_vidx = proposer20 ? host_lookup(c, proposer20) : -1;
  x.slot = c->x_issued & 1u;
  x.w = (uint32_t)(per / 64);
  x.total_words = x.w * c->xworld;
  x.seen_words = (c->n_validators + 63) / 64;
  x.n_pieces = 2 * c->power_words;
  x.slots = exchange_slots(K, x.w, c->xworld, c->n_validators);
  x.my_words = (uint32_t)mask_words(n_local);
  const uint64_t lo = std::min<uint64_t>((uint64_t)c->xrank * per, n_total), hi = std::min<uint64_t>(lo + per, n_total);
  if ((uint64_t)n_local != hi - lo) {
    c->last_error = "the resident batch is not this rank's shard of n_total rows (ibft_shard_range)";
    return IBFT_E_INVAL;
  }
  if (!c->d_seen_out.p) {
    c->last_error = "no tally has run since the context joined the exchange";
    return IBFT_E_INVAL;
  }
  int rc;
  if ((rc = ensure(c, c->d_xbuf[x.slot], (size_t)x.slots * 8))) return rc;
  const size_t res_words = (size_t)K * x.total_words + 16;
  if ((rc = ensure(c, c->d_xres[x.slot], res_words * 8))) return rc;
  if (res_words > c->h_xres_words) {  // (re)allocate the mapped result buffers; nothing is in flight on a fresh size
    if (c->x_issued != c->x_fetched) HIPCHK(c, hipStreamSynchronize(c->xstream));
    for (int i = 0; i < 2; i++) {
      if (c->h_xres[i]) (void)hipHostFree(c->h_xres[i]);
      c->h_xres[i] = c->dh_xres[i] = nullptr;
      if (hipHostMalloc((void **)&c->h_xres[i], res_words * 8) != hipSuccess) return IBFT_E_NOMEM;
      void *d = nullptr;
      if (hipHostGetDevicePointer(&d, c->h_xres[i], 0) == hipSuccess) c->dh_xres[i] = (uint64_t *)d;
    }
    c->h_xres_words = res_words;
  }
  if ((rc = ensure_handoff_events(c))) return rc;
  HIPCHK(c, hipEventRecord(c->ev_ready, c->stream));  // everything launched so far, the tally included
  HIPCHK(c, hipStreamWaitEvent(c->xstream, c->ev_ready, 0));
  ibftk::exchange_pack_args pa{};
  if (K == 2) {
    pa.mask[0] = (const uint64_t *)c->d_set.p;
    pa.mask[1] = (const uint64_t *)c->d_set.p + mask_words(c->max_rows);
  } else {
    pa.mask[0] = pa.mask[1] = (const uint64_t *)c->d_mask_out.p;
  }
  pa.seen = (const uint32_t *)c->d_seen_out.p;
  pa.tally_out = (const uint64_t *)c->d_tally.p;
  pa.xbuf = (uint64_t *)c->d_xbuf[x.slot].p;
  pa.K = K;
  pa.world = c->xworld;
  pa.rank = c->xrank;
  pa.words_per_rank = x.w;
  pa.my_words = x.my_words;
  pa.seen_words = x.seen_words;
  hipLaunchKernelGGL(ibftk::exchange_pack_kernel, dim3((x.slots + 255) / 256), dim3(256), 0, c->xstream, pa);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev_read, c->xstream));
  c->read_pending = true;  // the next tally overwrites d_mask_out / d_set / d_tally / d_seen_out only after the pack has read them
  return IBFT_OK;
}
int exchange_collective(ibft_ctx *c, RcclApi *api, const xplan &x) {
  NCCLCHK(c, api, api->AllReduce(c->d_xbuf[x.slot].p, c->d_xbuf[x.slot].p, x.slots, ncclUint64, ncclSum, c->comm, c->xstream));
  return IBFT_OK;
}
// The same step without a communicator: every rank's buffer is addressable from rank 0's device (one device listed
// several times, or peer access), so rank 0's exchange stream sums the buffers in place of ncclAllReduce — behind every
// rank's pack, in front of every rank's unpack.
int exchange_collective_local(const std::vector<ibft_ctx *> &ctx, const std::vector<xplan> &plan) {
  ibft_ctx *c0 = ctx[0];
  ibftk::exchange_sum_args sa{};
  sa.world = (uint32_t)ctx.size();
  sa.slots = plan[0].slots;
  for (size_t i = 0; i < ctx.size(); i++) {
    ibft_ctx *c = ctx[i];
    if (plan[i].slots != sa.slots) return IBFT_E_INVAL;
    sa.buf[i] = (uint64_t *)c->d_xbuf[plan[i].slot].p;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventRecord(c->ev_xpack, c->xstream));
  }
  HIPCHK(c0, hipSetDevice(c0->device));
  for (size_t i = 1; i < ctx.size(); i++) HIPCHK(c0, hipStreamWaitEvent(c0->xstream, ctx[i]->ev_xpack, 0));
  hipLaunchKernelGGL(ibftk::exchange_sum_kernel, dim3((sa.slots + 255) / 256), dim3(256), 0, c0->xstream, sa);
  HIPCHK(c0, hipGetLastError());
  HIPCHK(c0, hipEventRecord(c0->ev_xpack, c0->xstream));
  for (size_t i = 1; i < ctx.size(); i++) {
    HIPCHK(ctx[i], hipSetDevice(ctx[i]->device));
    HIPCHK(ctx[i], hipStreamWaitEvent(ctx[i]->xstream, c0->ev_xpack, 0));
  }
  return IBFT_OK;
}
int exchange_post(ibft_ctx *c, uint64_t n_total, const xplan &x) {
  HIPCHK(c, hipSetDevice(c->device));
  ibftk::exchange_unpack_args ua{};
  ua.xbuf = (const uint64_t *)c->d_xbuf[x.slot].p;
  ua.vpower32 = (const uint32_t *)c->d_vpower.p;
  ua.quorum = (const uint64_t *)c->d_quorum.p;
  ua.dst = (uint64_t *)c->d_xres[x.slot].p;
  ua.host_dst = c->dh_xres[x.slot];
  ua.K = x.K;
  ua.world = c->xworld;
  ua.words_per_rank = x.w;
  ua.seen_words = x.seen_words;
  ua.n_pieces = x.n_pieces;
  ua.n_validators = c->n_validators;
  ua.prop_on = x.prop_on ? 1u : 0u;
  ua.prop_vidx = x.prop_vidx;
  const uint32_t copy_blocks = (x.K * x.total_words + ibftk::XUNPACK_THREADS - 1) / ibftk::XUNPACK_THREADS;
  hipLaunchKernelGGL(ibftk::exchange_unpack_kernel, dim3(copy_blocks + 1), dim3(ibftk::XUNPACK_THREADS), 0, c->xstream, ua);
  HIPCHK(c, hipGetLastError());
  if (!c->dh_xres[x.slot])
    HIPCHK(c, hipMemcpyAsync(c->h_xres[x.slot], c->d_xres[x.slot].p, ((size_t)x.K * x.total_words + 16) * 8,
                             hipMemcpyDeviceToHost, c->xstream));
  HIPCHK(c, hipEventRecord(c->ev_xdone[x.slot], c->xstream));
  c->x_total[x.slot] = n_total;
  c->x_K[x.slot] = x.K;
  c->x_issued++;
  return IBFT_OK;
}
// out_mask: the first verdict array; out_mask2: the second one of a message-set exchange (K = 2)
int fetch_merged_locked(ibft_ctx *c, uint64_t *out_mask, ibft_tally_t *tally, uint64_t *out_mask2 = nullptr) {
  if (c->x_fetched == c->x_issued) return IBFT_E_INVAL;
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t slot = c->x_fetched & 1u;
  HIPCHK(c, hipEventSynchronize(c->ev_xdone[slot]));
  c->x_fetched++;
  if (c->cache_on && c->dh_tally) {  // keys this shard's rows taught the device (delivered by the tally kernel) → tables
    const uint32_t *lw = reinterpret_cast<const uint32_t *>(c->h_tally + 4);
    int rcb = build_new_tables(c, lw[0], lw[1]);
    if (rcb) return rcb;
  }
  const uint64_t n_total = c->x_total[slot];
  const uint32_t K = c->x_K[slot];
  const uint64_t per = shard_rows_per_rank(n_total, c->xworld);
  const size_t total_words = (size_t)(per / 64) * c->xworld, mw = (size_t)((n_total + 63) / 64);
  const uint64_t *res = c->h_xres[slot];
  if (out_mask && mw) memcpy(out_mask, res, mw * 8);
  if (out_mask2 && mw && K == 2) memcpy(out_mask2, res + total_words, mw * 8);
  const uint64_t *t = res + (size_t)K * total_words;
  for (int i = 0; i < ibftk::TALLY_SUM_WORDS; i++) c->last_wide[i] = t[4 + i];
  if (tally) {
    memset(tally, 0, sizeof *tally);
    tally->quorum_lo = c->quorum_w[0];
    tally->quorum_hi = c->quorum_w[1];
    tally->power_lo = t[0];
    tally->power_hi = t[1];
    tally->valid_rows = (uint32_t)(t[2] & 0xFFFFFFFFull);
    tally->distinct_senders = (uint32_t)(t[2] >> 32);
    tally->has_quorum = (uint32_t)t[3];
    tally->shard_overlap = (uint32_t)t[4 + ibftk::TALLY_SUM_WORDS];
    tally->proposer_rows = (uint32_t)t[5 + ibftk::TALLY_SUM_WORDS];
  }
  return IBFT_OK;
}
int comm_attach(ibft_ctx *c, ncclComm_t comm, uint32_t rank, uint32_t world) {
  HIPCHK(c, hipSetDevice(c->device));
  c->comm = comm;
  c->xlocal = comm == nullptr;
  c->xrank = rank;
  c->xworld = world;
  HIPCHK(c, hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking));
  for (int i = 0; i < 2; i++) HIPCHK(c, hipEventCreateWithFlags(&c->ev_xdone[i], hipEventDisableTiming));
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_xpack, hipEventDisableTiming));
  return IBFT_OK;
}

// One call of the device signer (ibft_sign_seals_ex, ibft_sign_messages_wire, ibft_sign_envelopes_wire), the context locked: what the
// three share around their own columns and kernels.  The secret keys go to d_payload (free during a signing call) and do not outlive
// the call in HBM: finish() zeroes them behind the last launch, the destructor on every way out between upload_keys() and finish().
struct sign_call {
  ibft_ctx *c;
  uint32_t nonce;
  size_t n;
  bool keys_up = false;
  ~sign_call() {
    if (!keys_up || !c->d_payload.p) return;
    (void)hipMemsetAsync(c->d_payload.p, 0, n * 32, c->stream);
    (void)hipStreamSynchronize(c->stream);
  }
  int check(const char *fn_name) {
    if (nonce != IBFT_SIGN_NONCE_KECCAK && nonce != IBFT_SIGN_NONCE_RFC6979) {
      c->last_error = std::string(fn_name) + ": unknown nonce rule " + std::to_string(nonce) + " (IBFT_SIGN_NONCE_KECCAK = 0, IBFT_SIGN_NONCE_RFC6979 = 1)";
      return IBFT_E_INVAL;
    }
    return n > c->max_rows ? IBFT_E_TOOBIG : IBFT_OK;
  }
  int begin() {
    HIPCHK(c, hipSetDevice(c->device));
    c->wire.columns = false;  // the columns used from here on are the wire walker's and the seal batch's
    c->staged_n = 0;
    return IBFT_OK;
  }
  int upload_keys(const uint8_t *sk32) {
    keys_up = true;  // (from here on: a copy that fails may have moved some of them)
    return upload(c, c->d_payload, sk32, n * 32);
  }
  uint32_t blocks() const { return (uint32_t)((n + ibftk::ROWS_PER_BLOCK - 1) / ibftk::ROWS_PER_BLOCK); }
  // a lane kernel of the signer, one wavefront per 64 rows, instantiated for the call's nonce rule: pick(N) names kernel<N>
  template <class Pick, class Args>
  void launch_signed(Pick pick, const Args &a) {
    with_int<ibftk::SIGN_NONCE_KECCAK, ibftk::SIGN_NONCE_RFC6979>((int)nonce, [&](auto N) {
      hipLaunchKernelGGL(pick(N), dim3(blocks()), dim3(ibftk::ROWS_PER_BLOCK), 0, c->stream, a);
    });
  }
  int finish(uint8_t *out_bytes, const void *d_bytes, size_t n_bytes, uint8_t *out_from20, uint8_t *out_ok) {
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync(c->d_payload.p, 0, n * 32, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_bytes, d_bytes, n_bytes, hipMemcpyDeviceToHost, c->stream));
    if (out_from20) HIPCHK(c, hipMemcpyAsync(out_from20, c->d_signer.p, n * 20, hipMemcpyDeviceToHost, c->stream));
    if (out_ok) HIPCHK(c, hipMemcpyAsync(out_ok, c->d_pre.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    keys_up = false;  // (zeroed, and the stream has drained)
    return IBFT_OK;
  }
};

}  // namespace

// One host thread per device of a group: staging and launching a shard costs tens of microseconds of host time per
// device, which one thread would pay W times in a row.
class GroupWorker {
 public:
  GroupWorker() : th_([this] { loop(); }) {}
  ~GroupWorker() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    th_.join();
  }
  void post(std::function<int()> fn) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      task_ = std::move(fn);
      busy_ = true;
    }
    cv_.notify_all();
  }
  int wait() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [this] { return !busy_; });
    return rc_;
  }

 private:
  void loop() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [this] { return stop_ || (busy_ && task_); });
      if (stop_) return;
      std::function<int()> fn = std::move(task_);
      task_ = nullptr;
      lk.unlock();
      const int rc = fn();
      lk.lock();
      rc_ = rc;
      busy_ = false;
      cv_.notify_all();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::function<int()> task_;
  bool busy_ = false, stop_ = false;
  int rc_ = 0;
  std::thread th_;
};

struct ibft_group {
  std::mutex mu;
  std::vector<ibft_ctx *> ctx;
  bool local = false;  // the collective is exchange_sum_kernel on rank 0's exchange stream, not ncclAllReduce
  std::vector<std::unique_ptr<GroupWorker>> worker;
  // run fn(i) for every rank on its own thread; the first non-zero return code (by rank) is the result
  int each(const std::function<int(uint32_t)> &fn) {
    if (ctx.size() == 1) return fn(0);
    for (uint32_t i = 0; i < ctx.size(); i++) worker[i]->post([&fn, i] { return fn(i); });
    int rc = IBFT_OK;
    for (uint32_t i = 0; i < ctx.size(); i++) {
      const int r = worker[i]->wait();
      if (r && !rc) rc = r;
    }
    return rc;
  }
};

extern "C" {

static void key_cache_unmap(ibft_ctx *c);

int ibft_version(void) { return 4; }  // 2: ibft_tally_t.proposer_rows, proposer20 arguments, ibft_tally_prepare, ibft_comm_info;
                                      // 3: ibft_seals_stage_next / _swap / _submit / _collect, ibft_last_cold_table, ibft_comm_preload, ibft_seals_rows, ibft_issue_probe;
                                      // 4: ibft_pipeline_stats (the side-stream tally of submitted passes changes no signature)

const char *ibft_strerror(int code) {
  switch (code) {
    case IBFT_OK: return "ok";
    case IBFT_E_INVAL: return "invalid argument";
    case IBFT_E_NODEVICE: return "no usable gfx950 device";
    case IBFT_E_NOMEM: return "out of memory";
    case IBFT_E_HIP: return "HIP runtime error";
    case IBFT_E_NOVALSET: return "validator set not configured";
    case IBFT_E_POWER: return "total voting power is zero or less";
    case IBFT_E_TOOBIG: return "batch exceeds max_rows";
    case IBFT_E_RCCL: return "RCCL unavailable or a collective failed";
    default: return "unknown error";
  }
}

// (NULL: why the calling thread's last ibft_ctx_create failed, where it left a reason — there is no context to ask then)
const char *ibft_last_error(const ibft_ctx *ctx) { return ctx ? ctx->last_error.c_str() : g_create_error.c_str(); }

int ibft_ctx_create(const ibft_cfg *cfg, ibft_ctx **out) {
  if (!out) return IBFT_E_INVAL;
  *out = nullptr;
  g_create_error.clear();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return IBFT_E_NODEVICE;
  int dev = cfg ? cfg->device : 0;
  if (dev < 0 || dev >= ndev) return IBFT_E_NODEVICE;
  if (hipSetDevice(dev) != hipSuccess) return IBFT_E_NODEVICE;
  // experiment: how much of a step is the host waking up?  IBFT_SPIN=1 asks the runtime to spin in synchronize calls
  if (const char *e = getenv("IBFT_SPIN"))
    if (atoi(e) == 1) (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return IBFT_E_NODEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return IBFT_E_NODEVICE;  // gfx950-only code object

  ibft_ctx *c = new (std::nothrow) ibft_ctx();
  if (!c) return IBFT_E_NOMEM;
  c->device = dev;
  c->flags = cfg ? cfg->flags : 0;
  c->max_rows = (cfg && cfg->max_rows) ? cfg->max_rows : DEFAULT_MAX_ROWS;
  c->kernel = cfg ? cfg->kernel : IBFT_KERNEL_AUTO;
  c->cold_group_auto = c->kernel != IBFT_KERNEL_LANE;
  if (const char *e = getenv("IBFT_SPLIT_LARGE")) c->split_large = strcmp(e, "0") != 0;
  if (const char *e = getenv("IBFT_SIDE_TALLY")) c->side_tally = strcmp(e, "0") == 0 ? 0 : strcmp(e, "1") == 0 ? 1 : 2;
  if (const char *e = getenv("IBFT_ALT_VERDICT")) c->alt_verdict = strcmp(e, "0") == 0 ? 0 : strcmp(e, "1") == 0 ? 1 : 2;
  if (const char *e = getenv("IBFT_COLD_TABLE")) {
    if (!strcmp(e, "lds")) c->cold_table_force = 1;
    else if (!strcmp(e, "private")) c->cold_table_force = 2;
    else if (!strcmp(e, "private2")) c->cold_table_force = 3;
  }
  if (const char *e = getenv("IBFT_COLD_LANES")) {
    const int g = atoi(e);
    if (g == 1 || g == 2 || g == 4 || g == 8 || g == 16 || g == 64 || g == 128) c->cold_group_force = (uint32_t)g;
  }
  if (const char *e = getenv("IBFT_WARM_LANES")) {
    const int g = atoi(e);
    if (g >= 1 && g <= 64 && (g & (g - 1)) == 0) c->warm_group_force = (uint32_t)g;
  }
  if (const char *e = getenv("IBFT_NO_EVENTS"))
    if (atoi(e) == 1) c->time_every = 0;
  if (getenv("IBFT_NO_GATHER")) c->gather_pinned = false;
  if (const char *e = getenv("IBFT_PROPOSAL_HASH")) c->hash_on_host = strcmp(e, "device") != 0;
  if (const char *e = getenv("IBFT_CERT_OVERLAP")) c->cert.overlap = atoi(e) != 0;
  c->cert.dedup = (c->flags & IBFT_FLAG_CERT_DEDUP) != 0;
  if (const char *e = getenv("IBFT_CERT_DEDUP")) c->cert.dedup = atoi(e) != 0;
  c->wire_recode = (c->flags & IBFT_FLAG_WIRE_RECODE) != 0;
  if (const char *e = getenv("IBFT_WIRE_RECODE")) c->wire_recode = atoi(e) != 0;
  if (const char *e = getenv("IBFT_CERT_DEDUP_SLOTS")) c->cert.dedup_slots_cap = (uint32_t)strtoul(e, nullptr, 10);
  if (const char *e = getenv("IBFT_WIRE_VIEWS_SLOTS")) c->wviews.slots_hook = (uint32_t)strtoul(e, nullptr, 10);
  if (const char *e = getenv("IBFT_ROUND_CHANGE_SLOTS")) c->cert.rc_slots_hook = (uint32_t)strtoul(e, nullptr, 10);
  {
    std::random_device rd;
    c->wviews.salt = (uint32_t)rd();
  }
  if (getenv("IBFT_DIGEST_FUSION")) c->digest_in_gather = true;
  if (const char *e = getenv("IBFT_WAVE_ROWS_MAX")) c->wave_rows_max = (uint32_t)strtoul(e, nullptr, 10);
  if (const char *e = getenv("IBFT_PAIR_ROWS_MAX")) c->pair_rows_max = (uint32_t)strtoul(e, nullptr, 10);
  if (const char *e = getenv("IBFT_ROWS_KERNEL_MAX")) c->rows_kernel_max = (uint32_t)strtoul(e, nullptr, 10);
  if (const char *e = getenv("IBFT_PROPOSAL_LANES")) {
    const int g = atoi(e);
    if (g == 1 || g == 64) c->proposal_lanes_force = (uint32_t)g;
  }
  if (const char *e = getenv("IBFT_STREAM_DIGEST")) c->stream_digest_copy = strcmp(e, "copy") == 0;
  if (const char *e = getenv("IBFT_ENVELOPE_LANES")) {
    const int g = atoi(e);
    if (g == 1 || g == 64) c->envelope_lanes_force = (uint32_t)g;
  }
  if (const char *e = getenv("IBFT_PROPOSAL_LANE_ROWS")) c->proposal_lane_rows = (uint32_t)strtoul(e, nullptr, 10);
  if (const char *e = getenv("IBFT_PROPOSAL_BYTES_MAX"))  // (offsets are 32-bit; room is kept for the round and the slack)
    c->proposal_bytes_max = std::min<uint64_t>(strtoull(e, nullptr, 10), 0xFFFFFE00ull);
  if (const char *e = getenv("IBFT_VALSETS_BYTES_MAX")) c->valsets_bytes_max = strtoull(e, nullptr, 10);
  if (const char *e = getenv("IBFT_ROWS_PAIR")) {
    if (!strcmp(e, "0")) c->rows_pair_force = 0;
    else if (!strcmp(e, "1")) c->rows_pair_force = 1;
  }
  c->compute_units = (uint32_t)prop.multiProcessorCount;
  if (const char *e = getenv("IBFT_PAIR_LEAVE")) {
    if (!strcmp(e, "0")) c->pair_leave_force = 0;
    else if (!strcmp(e, "1")) c->pair_leave_force = 1;
  }
  int rc = IBFT_OK;
  do {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = IBFT_E_HIP; break; }
    if (hipStreamCreateWithFlags(&c->hstream, hipStreamNonBlocking) != hipSuccess) { rc = IBFT_E_HIP; break; }
    if (hipEventCreateWithFlags(&c->ev_H, hipEventDisableTiming) != hipSuccess) { rc = IBFT_E_HIP; break; }
    if ((rc = alloc_rows(c, c->max_rows))) break;
    if (hipMemsetAsync(c->d_acc.p, 0, c->d_acc.cap, c->stream) != hipSuccess ||
        hipMemsetAsync(c->d_tally.p, 0, c->d_tally.cap, c->stream) != hipSuccess) { rc = IBFT_E_HIP; break; }
    if (hipHostMalloc((void **)&c->h_mask, (size_t)mask_words(c->max_rows) * 8 + 64) != hipSuccess) { rc = IBFT_E_NOMEM; break; }
    if (hipHostMalloc((void **)&c->h_tally, 128) != hipSuccess) { rc = IBFT_E_NOMEM; break; }
    if (hipHostMalloc((void **)&c->h_digest, 64) != hipSuccess) { rc = IBFT_E_NOMEM; break; }
    if (hipHostMalloc((void **)&c->h_set, (size_t)mask_words(c->max_rows) * 16 + 64) != hipSuccess) { rc = IBFT_E_NOMEM; break; }
    if ((rc = ensure(c, c->d_set, (size_t)mask_words(c->max_rows) * 16))) break;
    if (hipHostMalloc((void **)&c->h_class, (size_t)c->max_rows + 64) != hipSuccess) { rc = IBFT_E_NOMEM; break; }
    if ((rc = ensure(c, c->d_class, (size_t)c->max_rows + 64))) break;
    // zero-copy result delivery (tally_kernel writes the verdict words and its own result into the
    // pinned buffers); IBFT_NO_HOST_DIRECT=1 keeps the two device-to-host copies instead
    if (!getenv("IBFT_NO_HOST_DIRECT")) {
      void *dm = nullptr, *dt = nullptr;
      if (hipHostGetDevicePointer(&dm, c->h_mask, 0) == hipSuccess && hipHostGetDevicePointer(&dt, c->h_tally, 0) == hipSuccess) {
        c->dh_mask = (uint64_t *)dm;
        c->dh_tally = (uint64_t *)dt;
        void *ds = nullptr;
        if (hipHostGetDevicePointer(&ds, c->h_set, 0) == hipSuccess) c->dh_set = (uint64_t *)ds;
        void *dc = nullptr;
        if (hipHostGetDevicePointer(&dc, c->h_class, 0) == hipSuccess) c->dh_class = (uint8_t *)dc;
      }
    }
    {  // the device's shared object: created (and the G table built) by the first context of the device
      std::lock_guard<std::mutex> glk(g_devices_mu);
      c->dev = g_devices[c->device].lock();
      if (!c->dev) {
        const int form = qtab_form_from_env();
        if (form < 0) {
          g_create_error = std::string("IBFT_QTAB_FORM=") + getenv("IBFT_QTAB_FORM") + ": the key cache's table form is wide or glv";
          rc = IBFT_E_INVAL;
          break;
        }
        c->dev = std::make_shared<DeviceShared>();
        c->dev->device = c->device;
        c->dev->form = form;
        c->dev->slot_bytes = (form == ibftk::QTAB_GLV ? ibftk::QGLV_DWORDS_PER_VALIDATOR : ibftk::QTAB_DWORDS_PER_VALIDATOR) * 4;
        g_devices[c->device] = c->dev;
      }
    }
    {
      std::lock_guard<std::mutex> dlk(c->dev->mu);
      if (!c->dev->d_gtab.p) {
        if ((rc = ensure(c, c->dev->d_gtab, (size_t)ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES * ibftk::GTAB_ENTRY_DWORDS * 4))) break;
        int threads = 64, total = ibftk::GTAB_WINDOWS * ibftk::GTAB_ENTRIES;
        hipLaunchKernelGGL(ibftk::gtab_build_kernel, dim3((total + threads - 1) / threads), dim3(threads), 0,
                           c->stream, (uint32_t *)c->dev->d_gtab.p);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
          release(c->dev->d_gtab);
          rc = IBFT_E_HIP;
          break;
        }
      }
    }
  } while (0);
  if (rc) {
    ibft_ctx_destroy(c);
    return rc;
  }
  *out = c;
  return IBFT_OK;
}

void ibft_ctx_destroy(ibft_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->hstream) (void)hipStreamSynchronize(c->hstream);
  if (c->tstream) (void)hipStreamSynchronize(c->tstream);
  if (c->cstream) (void)hipStreamSynchronize(c->cstream);  // block batches in flight are drained, never delivered
  if (c->ostream) (void)hipStreamSynchronize(c->ostream);  // … their digests and emitted columns on the way out too
  for (DevBuf *b : {&c->d_hash, &c->d_sig, &c->d_signer, &c->d_signer_out, &c->d_pre, &c->d_hash_len, &c->d_payload,
                    &c->d_off, &c->d_raw, &c->d_mask, &c->d_mask_out, &c->d_vidx, &c->d_tally, &c->d_H,
                    &c->d_vtab, &c->d_vpower, &c->d_vslot,
                    &c->d_warm_done, &c->d_seen, &c->d_acc, &c->d_quorum, &c->d_wire_rows, &c->d_seal,
                    &c->d_xbuf[0], &c->d_xbuf[1], &c->d_xres[0], &c->d_xres[1], &c->d_set, &c->d_noseal, &c->d_class,
                    &c->d_hash_copy, &c->d_seen_out, &c->d_hash_nx, &c->d_sig_nx,
                    &c->d_signer_nx, &c->d_pre_nx, &c->d_mask_b, &c->d_vidx_b, &c->d_bhash, &c->d_boff, &c->brec.d,
                    &c->d_boff_nx, &c->d_praw, &c->d_proff, &c->d_pround,
                    &c->d_phash, &c->fam.d_vtab, &c->fam.d_vslot, &c->fam.d_setidx, &c->fam.d_meta, &c->fam.d_power,
                    &c->fam.d_quorum, &c->fam.d_seen, &c->fam.d_bset, &c->hsets.d_first, &c->hsets.d_range_set, &c->hsets.d_row_set,
                    &c->hsets.d_acc, &c->hsets.d_seen, &c->wviews.d_tables, &c->wviews.d_slots, &c->wviews.d_rank, &c->wviews.d_first,
                    &c->wviews.d_view, &c->wviews.d_stored, &c->wviews.d_acc, &c->wviews.d_recs, &c->wviews.d_sflags, &c->wviews.d_seal_row,
                    &c->wviews.d_seal_src, &c->wviews.d_seal_words, &c->wviews.d_seal_mask, &c->d_msg_cols, &c->d_msg_wire, &c->d_env_cols, &c->d_env_body, &c->d_env_wire})
    release(*b);
  if (c->h_phash) (void)hipHostFree(c->h_phash);
  if (c->tstream) {
    (void)hipStreamSynchronize(c->tstream);
    (void)hipStreamDestroy(c->tstream);
  }
  for (int i = 0; i < 2; i++)
    if (c->ev_rec[i]) (void)hipEventDestroy(c->ev_rec[i]);
  if (c->cstream) {
    (void)hipStreamSynchronize(c->cstream);
    (void)hipStreamDestroy(c->cstream);
  }
  if (c->ev_staged) (void)hipEventDestroy(c->ev_staged);
  if (c->ev_cols_read) (void)hipEventDestroy(c->ev_cols_read);
  if (c->ev_cols_read_b) (void)hipEventDestroy(c->ev_cols_read_b);
  if (c->dev) {
    {
      std::lock_guard<std::mutex> dlk(c->dev->mu);
      key_cache_unmap(c);
      family_view fv(c);  // … and the slots the family's union holds
      key_cache_unmap(c);
    }
    std::lock_guard<std::mutex> glk(g_devices_mu);
    if (c->dev.use_count() == 1) {  // the last context of the device: its tables go with it
      for (DevBuf *b : {&c->dev->d_gtab, &c->dev->d_pub, &c->dev->d_state, &c->dev->d_qtab, &c->dev->d_learned}) release(*b);
      g_devices.erase(c->device);
    }
    c->dev.reset();
  }
  c->cert.release_all();
  comm_release(c);
  if (c->ev_ready) (void)hipEventDestroy(c->ev_ready);
  if (c->ev_read) (void)hipEventDestroy(c->ev_read);
  for (int i = 0; i < 2; i++) {
    if (c->p_mask[i]) (void)hipHostFree(c->p_mask[i]);
    if (c->p_tally[i]) (void)hipHostFree(c->p_tally[i]);
    if (c->ev_pass[i]) (void)hipEventDestroy(c->ev_pass[i]);
  }
  if (c->h_mask) (void)hipHostFree(c->h_mask);
  if (c->brec.h) (void)hipHostFree(c->brec.h);
  for (BlockSlot &slot : c->bs) slot.release_all();
  if (c->ostream) (void)hipStreamDestroy(c->ostream);
  if (c->h_tally) (void)hipHostFree(c->h_tally);
  if (c->h_digest) (void)hipHostFree(c->h_digest);
  if (c->h_set) (void)hipHostFree(c->h_set);
  if (c->h_class) (void)hipHostFree(c->h_class);
  for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
  if (c->ev_H) (void)hipEventDestroy(c->ev_H);
  if (c->hstream) (void)hipStreamDestroy(c->hstream);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// powers: n × pw little-endian 64-bit words (pw = 1: ibft_set_validators, pw = 4: ibft_set_validators_u256)
// Drop this context's references to its slots; a slot nobody refers to any more is free for another address.
static void key_cache_unmap(ibft_ctx *c) {  // c->dev->mu held
  DeviceShared &d = *c->dev;
  for (uint32_t sl : c->vslot) {
    if (sl == 0xFFFFFFFFu || sl >= d.refs.size() || d.refs[sl] == 0) continue;
    if (--d.refs[sl] == 0) {
      d.slot_of.erase(d.addr_of[sl]);
      d.free_slots.push_back(sl);
    }
  }
  c->vslot.clear();
  c->my_built = 0;
  c->cache_on = false;
}

// Give every validator of the new set its slot (c->dev->mu held).  Grows the pool when the set needs more slots than it
// has (within IBFT_QTAB_BUDGET_GB, default 64: d.slot_bytes per slot — 655 KB wide, 174 KB GLV); validators beyond the budget
// simply have no slot.
static int key_cache_map(ibft_ctx *c, const std::vector<KeyAddr> &vaddr) {
  DeviceShared &d = *c->dev;
  const size_t nv = vaddr.size();
  if (nv == 0) {
    key_cache_unmap(c);
    return IBFT_E_INVAL;
  }
  // new references first, then the old ones go: an address in both sets never drops to zero in between
  std::vector<uint32_t> ns(nv, 0xFFFFFFFFu);
  size_t need_new = 0;
  for (size_t v = 0; v < nv; v++) {
    auto it = d.slot_of.find(vaddr[v]);
    if (it != d.slot_of.end()) {
      ns[v] = it->second;
      d.refs[it->second]++;
    } else {
      need_new++;
    }
  }
  {
    std::vector<uint32_t> old;
    old.swap(c->vslot);
    for (uint32_t sl : old) {
      if (sl == 0xFFFFFFFFu || d.refs[sl] == 0) continue;
      if (--d.refs[sl] == 0) {
        d.slot_of.erase(d.addr_of[sl]);
        d.free_slots.push_back(sl);
      }
    }
  }
  size_t budget = 64ull << 30;
  if (const char *e = getenv("IBFT_QTAB_BUDGET_GB")) budget = (size_t)strtoull(e, nullptr, 10) << 30;
  const size_t slot_bytes = d.slot_bytes;
  const size_t max_slots = budget / slot_bytes;
  const size_t avail = d.free_slots.size() + (d.cap - d.used);
  if (need_new > avail) {  // grow: the existing tables move to the new buffers (device copies), the pointers change
    size_t want = std::min(max_slots, std::max((size_t)d.used + (need_new - d.free_slots.size()), (size_t)d.cap * 2));
    if (want > d.cap) {
      DevBuf nq, np, nst;
      if (ensure(c, nq, want * slot_bytes) == IBFT_OK && ensure(c, np, want * ibftk::GTAB_ENTRY_DWORDS * 4) == IBFT_OK &&
          ensure(c, nst, want * 4) == IBFT_OK && (d.d_learned.p || ensure(c, d.d_learned, 8) == IBFT_OK)) {
        bool ok = hipMemset(nst.p, 0, want * 4) == hipSuccess;
        if (d.used) {
          ok = ok && hipMemcpy(nq.p, d.d_qtab.p, (size_t)d.used * slot_bytes, hipMemcpyDeviceToDevice) == hipSuccess;
          ok = ok && hipMemcpy(np.p, d.d_pub.p, (size_t)d.used * ibftk::GTAB_ENTRY_DWORDS * 4, hipMemcpyDeviceToDevice) == hipSuccess;
          ok = ok && hipMemcpy(nst.p, d.d_state.p, (size_t)d.used * 4, hipMemcpyDeviceToDevice) == hipSuccess;
        } else {
          ok = ok && hipMemset(d.d_learned.p, 0, 8) == hipSuccess;
        }
        if (ok) {
          release(d.d_qtab);   // (hipFree waits for every kernel of the device that may still read the old buffers;
          release(d.d_pub);    //  launches that would read the pointers take d.mu first, which we hold)
          release(d.d_state);
          d.d_qtab = nq;
          d.d_pub = np;
          d.d_state = nst;
          d.cap = (uint32_t)want;
          d.refs.resize(want, 0);
          d.addr_of.resize(want);
          d.built.resize(want, 0);
          d.generation++;
        } else {
          release(nq);
          release(np);
          release(nst);
        }
      } else {
        release(nq);
        release(np);
        release(nst);
      }
    }
  }
  std::vector<uint32_t> fresh;  // slots handed to new addresses: their state starts at 0
  for (size_t v = 0; v < nv; v++) {
    if (ns[v] != 0xFFFFFFFFu) continue;
    uint32_t sl;
    if (!d.free_slots.empty()) {
      sl = d.free_slots.back();
      d.free_slots.pop_back();
    } else if (d.used < d.cap) {
      sl = d.used++;
    } else {
      continue;  // beyond the budget: this validator stays on the recover path
    }
    d.slot_of[vaddr[v]] = sl;
    d.addr_of[sl] = vaddr[v];
    d.refs[sl] = 1;
    if (d.built[sl]) {
      d.built[sl] = 0;
      d.build_epoch++;
    }
    ns[v] = sl;
    fresh.push_back(sl);
  }
  if (d.cap == 0) {
    c->vslot.clear();
    return IBFT_E_NOMEM;
  }
  // a recycled slot must read "unknown" again before any kernel of this context can claim it
  std::sort(fresh.begin(), fresh.end());
  for (size_t i = 0; i < fresh.size();) {
    size_t j = i;
    while (j + 1 < fresh.size() && fresh[j + 1] == fresh[j] + 1) j++;
    HIPCHK(c, hipMemsetAsync((uint32_t *)d.d_state.p + fresh[i], 0, (j - i + 1) * 4, c->stream));
    i = j + 1;
  }
  int rc = ensure(c, c->d_vslot, nv * 4);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_vslot.p, ns.data(), nv * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->vslot.swap(ns);
  c->cache_on = true;
  c->seen_build_epoch = 0;
  recount_built(c);  // how many of THIS set's validators have a table already (all who stayed, any another context learned)
  return IBFT_OK;
}

// total voting power of nv validators (pw little-endian 64-bit words each) and quorum = ⌊2·total/3⌋ + 1 (calculateQuorum,
// validator_manager.go:130-135) in TALLY_SUM_WORDS × 64 bits, as 32-bit halves: total → ×2 → long division by 3 → +1.
// false: the total is zero (no quorum exists).
static bool quorum_words(const uint64_t *pwv, size_t nv, uint32_t pw, uint64_t quorum_w[ibftk::TALLY_SUM_WORDS]) {
  constexpr int H = 2 * ibftk::TALLY_SUM_WORDS;
  uint64_t piece[H] = {0};
  for (size_t v = 0; v < nv; v++)
    for (uint32_t k = 0; k < 2 * pw; k++) piece[k] += (pwv[v * pw + k / 2] >> (32 * (k & 1))) & 0xFFFFFFFFull;
  uint32_t half[H];
  {
    uint64_t carry = 0;
    for (int k = 0; k < H; k++) {
      const uint64_t t = carry + piece[k];
      half[k] = (uint32_t)t;
      carry = t >> 32;
    }
  }
  bool zero = true;
  for (int k = 0; k < H; k++) zero = zero && half[k] == 0;
  if (zero) return false;
  {
    uint32_t carry = 0;  // × 2
    for (int k = 0; k < H; k++) {
      const uint32_t top = half[k] >> 31;
      half[k] = (half[k] << 1) | carry;
      carry = top;
    }
    uint64_t rem = 0;    // ÷ 3
    for (int k = H - 1; k >= 0; k--) {
      const uint64_t cur = (rem << 32) | half[k];
      half[k] = (uint32_t)(cur / 3);
      rem = cur % 3;
    }
    for (int k = 0; k < H; k++)  // + 1
      if (++half[k] != 0) break;
  }
  for (int i = 0; i < ibftk::TALLY_SUM_WORDS; i++) quorum_w[i] = (uint64_t)half[2 * i] | ((uint64_t)half[2 * i + 1] << 32);
  return true;
}

static int set_validators_impl(ibft_ctx *c, uint64_t height, const uint8_t *addrs20, const uint64_t *power, uint32_t pw,
                               size_t n) {
  ctx_lock lk(c);
  HIPCHK(c, hipSetDevice(c->device));
  // Host-side build of the open-addressing table; a repeated address keeps the LAST
  // power (a Go map assignment in a loop), mirroring oracle/ibft_oracle.c.
  uint32_t slots = 64;
  while (slots < 2 * n + 2) slots <<= 1;
  std::vector<uint32_t> tab((size_t)slots * 6, 0);
  std::vector<uint64_t> pwv;  // distinct validators × pw words
  pwv.reserve((n ? n : 1) * pw);
  std::vector<KeyAddr> vaddr;  // distinct validators' addresses, by validator index
  vaddr.reserve(n);
  for (size_t i = 0; i < n; i++) {
    uint32_t a[5];
    memcpy(a, addrs20 + 20 * i, 20);
    uint32_t s = ibftk::addr_hash(a) & (slots - 1);
    for (;;) {
      uint32_t *e = &tab[(size_t)s * 6];
      if (e[5] == 0) {
        memcpy(e, a, 20);
        pwv.insert(pwv.end(), power + i * pw, power + (i + 1) * pw);
        e[5] = (uint32_t)(pwv.size() / pw);
        KeyAddr ka;
        memcpy(ka.b, a, 20);
        vaddr.push_back(ka);  // address of validator index e[5] − 1
        break;
      }
      if (memcmp(e, a, 20) == 0) {
        memcpy(&pwv[(size_t)(e[5] - 1) * pw], power + i * pw, (size_t)pw * 8);
        break;
      }
      s = (s + 1) & (slots - 1);
    }
  }
  const size_t nv = pwv.size() / pw;
  uint64_t quorum_w[ibftk::TALLY_SUM_WORDS];
  if (!quorum_words(pwv.data(), nv, pw, quorum_w)) return IBFT_E_POWER;  // validator_manager.go:68-70
  int rc;
  if ((rc = upload(c, c->d_vtab, tab.data(), tab.size() * 4))) return rc;
  if ((rc = upload(c, c->d_vpower, pwv.data(), pwv.size() * 8))) return rc;
  if ((rc = upload(c, c->d_quorum, quorum_w, sizeof quorum_w))) return rc;
  const size_t seen_bytes = ((nv + 31) / 32) * 4;
  if (seen_bytes > c->d_seen.cap) {  // the tally keeps the bitmap zeroed between launches: zero it when it is (re)allocated
    if ((rc = ensure(c, c->d_seen, seen_bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_seen.p, 0, c->d_seen.cap, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // warm path: the validators of this set get their slots in the device's key cache — an address that had one keeps it
  // (and its table), whatever changed around it
  if (c->flags & IBFT_FLAG_PUBKEY_CACHE) {
    std::lock_guard<std::mutex> dlk(c->dev->mu);
    c->cache_on = key_cache_map(c, vaddr) == IBFT_OK;
  }
  c->valset_addrs.assign(addrs20, addrs20 + n * 20);
  c->h_vtab = std::move(tab);
  c->vslot_mask = slots - 1;
  c->n_validators = (uint32_t)nv;
  c->power_words = pw;
  memcpy(c->quorum_w, quorum_w, sizeof quorum_w);
  c->height = height;
  c->have_valset = true;
  return IBFT_OK;
}

int ibft_set_validators(ibft_ctx *c, uint64_t height, const uint8_t *addrs20, const uint64_t *power, size_t n) {
  if (!c || (n && (!addrs20 || !power)) || n > (1u << 20)) return IBFT_E_INVAL;
  return set_validators_impl(c, height, addrs20, power, 1, n);
}

int ibft_set_validators_u256(ibft_ctx *c, uint64_t height, const uint8_t *addrs20, const uint8_t *power_be32, size_t n) {
  if (!c || (n && (!addrs20 || !power_be32)) || n > (1u << 20)) return IBFT_E_INVAL;
  std::vector<uint64_t> words(n * 4);  // big.Int.FillBytes(32) → four little-endian words
  for (size_t i = 0; i < n; i++)
    for (int w = 0; w < 4; w++) {
      uint64_t v = 0;
      for (int b = 0; b < 8; b++) v = (v << 8) | power_be32[32 * i + 8 * (3 - w) + b];
      words[4 * i + w] = v;
    }
  return set_validators_impl(c, height, addrs20, words.data(), 4, n);
}

// ---- a family of validator sets: the union's table, setidx[s][u], per-set powers / quorum / size ---------------------------
// Everything that can refuse is decided on the host before the device is touched, and the new tables are complete in buffers
// of their own before the old family is let go: a refused install leaves the previous family as it was.
static int check_validator_sets_args(const ibft_ctx *c, size_t n_sets, const uint32_t *set_off, const void *addrs20, const void *power) {
  if (!c || n_sets == 0 || !set_off || set_off[0] != 0) return IBFT_E_INVAL;
  for (size_t s = 0; s < n_sets; s++)
    if (set_off[s + 1] < set_off[s]) return IBFT_E_INVAL;
  if (set_off[n_sets] && (!addrs20 || !power)) return IBFT_E_INVAL;
  return IBFT_OK;
}

static int set_validator_sets_impl(ibft_ctx *c, size_t n_sets, const uint32_t *set_off, const uint8_t *addrs20, const uint64_t *power,
                                   uint32_t pw) {
  for (size_t s = 0; s < n_sets; s++)
    if (set_off[s + 1] - set_off[s] > c->max_rows) return IBFT_E_TOOBIG;
  // union index of an address: the order of first appearance over the whole family.  Within a set a repeated address keeps
  // its FIRST position and its LAST power, as in set_validators_impl.
  std::unordered_map<KeyAddr, uint32_t, KeyAddrHash> union_of;
  std::vector<KeyAddr> uaddr;
  std::vector<uint32_t> stamp, pos;     // by union index: the last set that listed it (+1), its index in that set
  std::vector<uint32_t> member_u;       // the sets' distinct members, set after set, as union indices
  std::vector<uint64_t> pwv;            // … and their powers, pw words each
  std::vector<uint32_t> pbase(n_sets + 1, 0);
  member_u.reserve(set_off[n_sets]);
  pwv.reserve((size_t)set_off[n_sets] * pw);
  for (size_t s = 0; s < n_sets; s++) {
    pbase[s] = (uint32_t)member_u.size();
    for (uint32_t i = set_off[s]; i < set_off[s + 1]; i++) {
      KeyAddr ka;
      memcpy(ka.b, addrs20 + 20ull * i, 20);
      auto it = union_of.find(ka);
      uint32_t u;
      if (it == union_of.end()) {
        u = (uint32_t)uaddr.size();
        if (u >= c->max_rows) return IBFT_E_TOOBIG;
        union_of.emplace(ka, u);
        uaddr.push_back(ka);
        stamp.push_back(0);
        pos.push_back(0);
      } else {
        u = it->second;
      }
      if (stamp[u] == (uint32_t)s + 1) {
        memcpy(&pwv[((size_t)pbase[s] + pos[u]) * pw], power + (size_t)i * pw, (size_t)pw * 8);
        continue;
      }
      stamp[u] = (uint32_t)s + 1;
      pos[u] = (uint32_t)member_u.size() - pbase[s];
      member_u.push_back(u);
      pwv.insert(pwv.end(), power + (size_t)i * pw, power + (size_t)(i + 1) * pw);
    }
  }
  pbase[n_sets] = (uint32_t)member_u.size();
  const size_t nu = uaddr.size();
  uint32_t slots = 64, largest = 0;
  while (slots < 2 * nu + 2) slots <<= 1;
  for (size_t s = 0; s < n_sets; s++) largest = std::max(largest, pbase[s + 1] - pbase[s]);
  const size_t seen_bytes = std::max<size_t>(((size_t)(largest + 31) / 32) * 4, 4);
  const uint64_t setidx_bytes = (uint64_t)n_sets * nu * 4;
  const uint64_t bytes = (uint64_t)slots * 24 + setidx_bytes + (uint64_t)n_sets * 8 + (uint64_t)pwv.size() * 8 +
                         (uint64_t)n_sets * ibftk::TALLY_SUM_WORDS * 8 + seen_bytes;
  if (bytes > c->valsets_bytes_max) return IBFT_E_TOOBIG;
  std::vector<uint64_t> quorum(n_sets * ibftk::TALLY_SUM_WORDS);
  for (size_t s = 0; s < n_sets; s++)  // an empty set included: its total is zero
    if (!quorum_words(pwv.data() + (size_t)pbase[s] * pw, pbase[s + 1] - pbase[s], pw, &quorum[s * ibftk::TALLY_SUM_WORDS]))
      return IBFT_E_POWER;
  std::vector<uint32_t> tab((size_t)slots * 6, 0);
  for (size_t u = 0; u < nu; u++) {
    uint32_t a[5];
    memcpy(a, uaddr[u].b, 20);
    uint32_t sl = ibftk::addr_hash(a) & (slots - 1);
    while (tab[(size_t)sl * 6 + 5] != 0) sl = (sl + 1) & (slots - 1);
    memcpy(&tab[(size_t)sl * 6], a, 20);
    tab[(size_t)sl * 6 + 5] = (uint32_t)u + 1;
  }
  std::vector<int32_t> setidx((size_t)n_sets * nu, -1);
  std::vector<uint32_t> meta(n_sets * 2);
  for (size_t s = 0; s < n_sets; s++) {
    meta[2 * s] = pbase[s];
    meta[2 * s + 1] = pbase[s + 1] - pbase[s];
    for (uint32_t k = pbase[s]; k < pbase[s + 1]; k++) setidx[s * nu + member_u[k]] = (int32_t)(k - pbase[s]);
  }

  ctx_lock lk(c);
  HIPCHK(c, hipSetDevice(c->device));
  ValFamily nf;
  DevBuf *fresh[] = {&nf.d_vtab, &nf.d_setidx, &nf.d_meta, &nf.d_power, &nf.d_quorum, &nf.d_seen};
  int rc = IBFT_OK;
  if (!(rc = upload(c, nf.d_vtab, tab.data(), tab.size() * 4)) && !(rc = upload(c, nf.d_setidx, setidx.data(), setidx.size() * 4)) &&
      !(rc = upload(c, nf.d_meta, meta.data(), meta.size() * 4)) && !(rc = upload(c, nf.d_power, pwv.data(), pwv.size() * 8)) &&
      !(rc = upload(c, nf.d_quorum, quorum.data(), quorum.size() * 8)) && !(rc = ensure(c, nf.d_seen, seen_bytes))) {
    // The wait for the MAIN stream is more than the end of these uploads: the kernels of streamed _sets batches in flight
    // read the old family's tables and the key-cache slots of its union, and every one of them runs on the main stream
    // (block_seals_submit_impl).  The release of the old buffers and key_cache_map below — which drops or remaps the old
    // union's references — rely on it.
    if (hipMemsetAsync(nf.d_seen.p, 0, nf.d_seen.cap, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
      c->last_error = "ibft_set_validator_sets: upload failed";
      rc = IBFT_E_HIP;
    }
  }
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    for (DevBuf *b : fresh) release(*b);
    return rc;
  }
  // The new family is whole: the old one goes.  Streamed _sets batches may be in flight (their results sit in their slots
  // and stay collectable: what a collect delivers is the slot's, nothing of c->fam); the wait above is what lets it go.
  ValFamily &f = c->fam;
  std::swap(f.d_vtab, nf.d_vtab);
  std::swap(f.d_setidx, nf.d_setidx);
  std::swap(f.d_meta, nf.d_meta);
  std::swap(f.d_power, nf.d_power);
  std::swap(f.d_quorum, nf.d_quorum);
  std::swap(f.d_seen, nf.d_seen);
  for (DevBuf *b : fresh) release(*b);
  f.vslot_mask = slots - 1;
  f.n_union = (uint32_t)nu;
  f.n_sets = (uint32_t)n_sets;
  f.power_words = pw;
  f.largest_set = largest;
  f.entries = pbase[n_sets];
  f.quorum.swap(quorum);
  f.have = true;
  // the height map named sets of the family that just went (the wait above covers whatever read it)
  c->hsets.have = false;
  c->hsets.n_ranges = 0;
  // warm path: the union's addresses hold key-cache slots while the family is installed — references of their own, next to
  // those of the context's single set; an address the previous family held keeps its slot and its table
  if (c->flags & IBFT_FLAG_PUBKEY_CACHE) {
    family_view fv(c);
    std::lock_guard<std::mutex> dlk(c->dev->mu);
    c->cache_on = key_cache_map(c, uaddr) == IBFT_OK;
  }
  f.device_bytes = f.d_vtab.cap + f.d_setidx.cap + f.d_meta.cap + f.d_power.cap + f.d_quorum.cap + f.d_seen.cap + f.d_vslot.cap;
  return IBFT_OK;
}

int ibft_set_validator_sets(ibft_ctx *c, size_t n_sets, const uint64_t *height, const uint32_t *set_off, const uint8_t *addrs20,
                            const uint64_t *power) {
  (void)height;  // informational
  int rc = check_validator_sets_args(c, n_sets, set_off, addrs20, power);
  if (rc) return rc;
  return set_validator_sets_impl(c, n_sets, set_off, addrs20, power, 1);
}

int ibft_set_validator_sets_u256(ibft_ctx *c, size_t n_sets, const uint64_t *height, const uint32_t *set_off, const uint8_t *addrs20,
                                 const uint8_t *power_be32) {
  (void)height;
  int rc = check_validator_sets_args(c, n_sets, set_off, addrs20, power_be32);
  if (rc) return rc;
  for (size_t s = 0; s < n_sets; s++)  // (before the powers are converted: a list beyond max_rows is not walked)
    if (set_off[s + 1] - set_off[s] > c->max_rows) return IBFT_E_TOOBIG;
  const size_t n = set_off[n_sets];
  std::vector<uint64_t> words(n * 4);  // big.Int.FillBytes(32) → four little-endian words
  for (size_t i = 0; i < n; i++)
    for (int w = 0; w < 4; w++) {
      uint64_t v = 0;
      for (int b = 0; b < 8; b++) v = (v << 8) | power_be32[32 * i + 8 * (3 - w) + b];
      words[4 * i + w] = v;
    }
  return set_validator_sets_impl(c, n_sets, set_off, addrs20, words.data(), 4);
}

int ibft_validator_sets_info(ibft_ctx *c, uint32_t *n_sets, uint32_t *union_size, uint64_t *device_bytes) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (n_sets) *n_sets = c->fam.have ? c->fam.n_sets : 0;
  if (union_size) *union_size = c->fam.have ? c->fam.n_union : 0;
  // + the calls' block_set column, and those of the two slots of the streamed _sets submits
  if (device_bytes) *device_bytes = c->fam.have ? c->fam.device_bytes + c->fam.d_bset.cap + c->bs[0].block_set_bytes() + c->bs[1].block_set_bytes() : 0;
  return IBFT_OK;
}

// ---- the height map of the live route under a family: heights [first_height[k], first_height[k + 1]) → set range_set[k] --------
// The new map is complete in buffers of its own before the old one goes: a refused install leaves the old map in place.  Its
// only reader is ibft_verify_senders_wire_sets, which has synchronised before it returned.
int ibft_set_height_sets(ibft_ctx *c, size_t n_ranges, const uint64_t *first_height, const uint32_t *range_set) {
  if (!c) return IBFT_E_INVAL;
  if (n_ranges == 0) {
    ctx_lock lk(c);
    c->hsets.have = false;
    c->hsets.n_ranges = 0;
    return IBFT_OK;
  }
  if (!first_height || !range_set) return IBFT_E_INVAL;
  for (size_t k = 0; k < n_ranges; k++)
    if (first_height[k + 1] <= first_height[k]) return IBFT_E_INVAL;
  if (n_ranges > IBFT_HEIGHT_RANGES_MAX) return IBFT_E_TOOBIG;
  ctx_lock lk(c);
  const ValFamily &f = c->fam;
  if (!f.have) return IBFT_E_NOVALSET;
  for (size_t k = 0; k < n_ranges; k++)
    if (range_set[k] >= f.n_sets) return IBFT_E_INVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HeightSets &h = c->hsets;
  DevBuf nfirst, nset;
  const size_t acc_bytes = (size_t)f.n_sets * (2 * f.power_words + 1) * 8, seen_bytes = std::max<size_t>(((size_t)f.entries + 31) / 32 * 4, 4);
  int rc;
  if (!(rc = upload(c, nfirst, first_height, (n_ranges + 1) * 8)) && !(rc = upload(c, nset, range_set, n_ranges * 4)) &&
      !(rc = ensure(c, h.d_acc, acc_bytes)) && !(rc = ensure(c, h.d_seen, seen_bytes)) &&
      !(rc = ensure(c, h.d_row_set, (size_t)c->max_rows * 4))) {
    if (hipMemsetAsync(h.d_acc.p, 0, h.d_acc.cap, c->stream) != hipSuccess || hipMemsetAsync(h.d_seen.p, 0, h.d_seen.cap, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
      c->last_error = "ibft_set_height_sets: upload failed";
      rc = IBFT_E_HIP;
    }
  }
  if (rc) {  // (the scratch buffers may have been re-allocated: without them the old map cannot be used either)
    (void)hipStreamSynchronize(c->stream);
    release(nfirst);
    release(nset);
    if (!h.d_acc.p || !h.d_seen.p || !h.d_row_set.p) h.have = false;
    return rc;
  }
  std::swap(h.d_first, nfirst);
  std::swap(h.d_range_set, nset);
  release(nfirst);
  release(nset);
  h.n_ranges = (uint32_t)n_ranges;
  h.lo = first_height[0];
  h.hi = first_height[n_ranges];
  h.have = true;
  return IBFT_OK;
}

int ibft_height_sets_info(ibft_ctx *c, uint32_t *n_ranges, uint64_t *lo, uint64_t *hi) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  const HeightSets &h = c->hsets;
  if (n_ranges) *n_ranges = h.have ? h.n_ranges : 0;
  if (lo) *lo = h.have ? h.lo : 0;
  if (hi) *hi = h.have ? h.hi : 0;
  return IBFT_OK;
}

int ibft_last_tally_wide(ibft_ctx *c, ibft_tally_wide_t *out) {
  if (!c || !out) return IBFT_E_INVAL;
  ctx_lock lk(c);
  memset(out, 0, sizeof *out);
  for (int i = 0; i < ibftk::TALLY_SUM_WORDS; i++) {
    out->quorum[i] = c->quorum_w[i];
    out->power[i] = c->last_wide[i];
  }
  bool ge = true;
  for (int i = ibftk::TALLY_SUM_WORDS - 1; i >= 0; i--)
    if (out->power[i] != out->quorum[i]) {
      ge = out->power[i] > out->quorum[i];
      break;
    }
  out->has_quorum = ge ? 1 : 0;
  return IBFT_OK;
}

int ibft_keccak256(const uint8_t *a, size_t na, const uint8_t *b, size_t nb, uint8_t out32[32]) {
  if (!out32 || (na && !a) || (nb && !b)) return IBFT_E_INVAL;
  host_keccak256(a, na, b, nb, out32);
  return IBFT_OK;
}

int ibft_proposal_hash(ibft_ctx *c, const uint8_t *raw, size_t raw_len, uint64_t round, uint8_t out32[32]) {
  if (!c || (raw_len && !raw) || !out32 || raw_len > (1ull << 31)) return IBFT_E_INVAL;
  ctx_lock lk(c);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_proposal_hash(c, raw, raw_len, round))) return rc;
  if (c->have_H && c->have_H_host) {  // hashed on the host: the digest is at hand (d_H receives it on the side stream)
    memcpy(out32, c->H_host, 32);
    return IBFT_OK;
  }
  if ((rc = wait_proposal_hash(c))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->h_digest, c->d_H.p, 32, hipMemcpyDeviceToHost, c->stream));
  if (hipStreamSynchronize(c->stream) != hipSuccess) {
    c->have_H = false;
    c->last_error = "hipStreamSynchronize failed";
    return IBFT_E_HIP;
  }
  memcpy(out32, c->h_digest, 32);
  return IBFT_OK;
}

static int hash_eq_locked(ibft_ctx *c, const uint8_t *hash32, const uint8_t *hash_len, size_t n, uint64_t *out_mask) {
  int rc;
  c->wire.columns = false;
  if ((rc = wait_proposal_hash(c))) return rc;
  ColumnCopies cc;
  cc.add(c->d_hash.p, hash32, n * 32);
  cc.add(c->d_hash_len.p, hash_len, n);
  if ((rc = cc.flush(c))) return rc;
  if (n) {
    hipLaunchKernelGGL(ibftk::hash_eq_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       (const uint8_t *)c->d_hash.p, (const uint8_t *)c->d_hash_len.p,
                       (const uint64_t *)c->d_H.p, (uint32_t)n, (uint64_t *)c->d_mask.p);
    HIPCHK(c, hipGetLastError());
    c->mask_dirty_words = std::max(c->mask_dirty_words, (uint32_t)mask_words(n));  // ballot words, no tally follows
  }
  rc = fetch_results(c, (uint32_t)n, out_mask, nullptr, false);
  if (rc) c->have_H = false;  // a failed stream leaves nothing to trust
  return rc;
}

int ibft_forget_proposal(ibft_ctx *c) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  c->have_H = false;
  return IBFT_OK;
}

int ibft_verify_hashes(ibft_ctx *c, const uint8_t *raw, size_t raw_len, uint64_t round,
                       const uint8_t *hash32, const uint8_t *hash_len, size_t n, uint64_t *out_mask) {
  if (!c || (raw_len && !raw) || (n && (!hash32 || !hash_len || !out_mask)) || raw_len > (1ull << 31))
    return IBFT_E_INVAL;
  ctx_lock lk(c);  // context state is only read inside the critical section
  if (n > c->max_rows) return IBFT_E_TOOBIG;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_proposal_hash(c, raw, raw_len, round))) return rc;
  return hash_eq_locked(c, hash32, hash_len, n, out_mask);
}

int ibft_verify_hashes_digest(ibft_ctx *c, const uint8_t digest32[32], const uint8_t *hash32, const uint8_t *hash_len,
                              size_t n, uint64_t *out_mask) {
  if (!c || !digest32 || (n && (!hash32 || !hash_len || !out_mask))) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (n > c->max_rows) return IBFT_E_TOOBIG;
  HIPCHK(c, hipSetDevice(c->device));
  {
    int rcw = wait_proposal_hash(c);  // a hash still on its way must not land on top of the caller's digest
    if (rcw) return rcw;
  }
  c->have_H = false;  // d_H now holds the caller's digest, not the hash of the remembered proposal
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging buffer is free again
  memcpy(c->h_digest, digest32, 32);
  HIPCHK(c, hipMemcpyAsync(c->d_H.p, c->h_digest, 32, hipMemcpyHostToDevice, c->stream));
  return hash_eq_locked(c, hash32, hash_len, n, out_mask);
}

// bare: the rows are bare seals (ibft_recover_seals) — there is no signer column to stage
static int seals_stage_locked(ibft_ctx *c, const uint8_t *hash32, const uint8_t *sig65, const uint8_t *signer20,
                              const uint8_t *pre_flags, size_t n, bool wait, bool bare = false) {
  if (n && (!hash32 || !sig65 || (!bare && !signer20))) return IBFT_E_INVAL;
  if (n > c->max_rows) return IBFT_E_TOOBIG;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  c->wire.columns = false;
  ColumnCopies cc;
  cc.add(c->d_hash.p, hash32, n * 32);
  cc.add(c->d_sig.p, sig65, n * 65);
  if (!bare) cc.add(c->d_signer.p, signer20, n * 20);
  if (pre_flags) cc.add(c->d_pre.p, pre_flags, n);
  if ((rc = cc.flush(c))) return rc;
  if ((rc = apply_seal_digest(c, c->d_hash.p, (uint32_t)n))) return rc;
  // ibft_seals_stage promises the caller its buffers back; the one-shot call waits once, at the end
  if (wait) HIPCHK(c, hipStreamSynchronize(c->stream));
  c->staged_n = (uint32_t)n;
  c->staged_pre = pre_flags != nullptr;
  return IBFT_OK;
}

int ibft_seals_stage(ibft_ctx *c, const uint8_t *hash32, const uint8_t *sig65, const uint8_t *signer20,
                     const uint8_t *pre_flags, size_t n) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  return seals_stage_locked(c, hash32, sig65, signer20, pre_flags, n, true);
}

// The copy stream with its two events and the spare set of seal columns, on first use (ibft_seals_stage_next,
// ibft_block_seals_submit)
static int ensure_spare_columns(ibft_ctx *c) {
  if (!c->cstream) {
    HIPCHK(c, hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_staged, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_cols_read, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_cols_read, c->stream));
  }
  int rc;
  const size_t m = std::max<size_t>(c->max_rows, c->row_cap);
  if ((rc = ensure(c, c->d_hash_nx, m * 32))) return rc;
  if ((rc = ensure(c, c->d_sig_nx, m * 65 + 64))) return rc;
  if ((rc = ensure(c, c->d_signer_nx, m * 20))) return rc;
  if ((rc = ensure(c, c->d_pre_nx, m))) return rc;
  return IBFT_OK;
}

// Double-buffered staging: the copy of batch k+1 overlaps the verdict kernels of batch k.
int ibft_seals_stage_next(ibft_ctx *c, const uint8_t *hash32, const uint8_t *sig65, const uint8_t *signer20,
                          const uint8_t *pre_flags, size_t n) {
  if (!c || (n && (!hash32 || !sig65 || !signer20))) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself: no join_side)
  if (n > c->max_rows) return IBFT_E_TOOBIG;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_spare_columns(c))) return rc;
  // the spare slot was the resident one until the last swap: kernels enqueued before that swap may still read it
  HIPCHK(c, hipStreamWaitEvent(c->cstream, c->ev_cols_read, 0));
  if (c->ev_cols_read_b) HIPCHK(c, hipStreamWaitEvent(c->cstream, c->ev_cols_read_b, 0));
  if (n) {
    HIPCHK(c, hipMemcpyAsync(c->d_hash_nx.p, hash32, n * 32, hipMemcpyHostToDevice, c->cstream));
    HIPCHK(c, hipMemcpyAsync(c->d_sig_nx.p, sig65, n * 65, hipMemcpyHostToDevice, c->cstream));
    HIPCHK(c, hipMemcpyAsync(c->d_signer_nx.p, signer20, n * 20, hipMemcpyHostToDevice, c->cstream));
    if (pre_flags) HIPCHK(c, hipMemcpyAsync(c->d_pre_nx.p, pre_flags, n, hipMemcpyHostToDevice, c->cstream));
  }
  HIPCHK(c, hipEventRecord(c->ev_staged, c->cstream));
  c->next_n = (uint32_t)n;
  c->next_pre = pre_flags != nullptr;
  c->next_valid = true;
  return IBFT_OK;
}

int ibft_seals_swap(ibft_ctx *c, int wait_for_copy) {
  if (!c) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself: no join_side)
  if (!c->next_valid) {
    c->last_error = "ibft_seals_swap without a batch staged by ibft_seals_stage_next";
    return IBFT_E_INVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  // everything enqueued so far read the columns that become the spare slot now; what is enqueued from here on reads the
  // other set, once its copy has landed (a device-side wait: the host does not block unless asked to)
  HIPCHK(c, hipEventRecord(c->ev_cols_read, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_staged, 0));
  // ... on either verdict stream: hstream's launches so far are readers of the old set too, its next ones of the new
  if (c->alt_used) {
    if (!c->ev_cols_read_b) HIPCHK(c, hipEventCreateWithFlags(&c->ev_cols_read_b, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_cols_read_b, c->hstream));
  }
  if (c->alt_verdict != 0) HIPCHK(c, hipStreamWaitEvent(c->hstream, c->ev_staged, 0));
  if (c->seal_digest_mode != 0) c->main_touched = true;  // (apply_seal_digest below rewrites the hash column on the main stream)
  std::swap(c->d_hash, c->d_hash_nx);
  std::swap(c->d_sig, c->d_sig_nx);
  std::swap(c->d_signer, c->d_signer_nx);
  std::swap(c->d_pre, c->d_pre_nx);
  c->staged_n = c->next_n;
  c->staged_pre = c->next_pre;
  c->next_valid = false;
  c->wire.columns = false;
  int rc;
  if ((rc = apply_seal_digest(c, c->d_hash.p, c->staged_n))) return rc;
  if (wait_for_copy) HIPCHK(c, hipEventSynchronize(c->ev_staged));  // the caller's source buffers are free again
  return IBFT_OK;
}

static int seals_launch_locked(ibft_ctx *c, uint32_t repeat, int mode = ibftk::MODE_SEALS) {
  if (!c->have_valset) return IBFT_E_NOVALSET;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->ev_used >= 4096) c->ev_used = 0;  // event pairs accumulate until ibft_last_kernel_ms reads (and resets) them
  if (repeat == 0) repeat = 1;
  c->launched_n = c->staged_n;
  for (uint32_t k = 0; k < repeat; k++) {
    int rc;
    const bool time_it = c->time_every && (c->pass_counter++ % c->time_every) == 0;
    if ((rc = enqueue_recover(c, c->stream, c->staged_n, c->staged_pre, mode, time_it))) return rc;
    if ((rc = enqueue_tally(c, c->staged_n))) return rc;
  }
  return IBFT_OK;
}

// mapped result slots (the tally kernel writes them itself) and the pass events, on first use — piece by piece, so that a
// failure half way leaves nothing to leak and nothing half set up for the next call (ibft_seals_submit, ibft_block_seals_submit)
static int ensure_result_slots(ibft_ctx *c) {
  for (int i = 0; i < 2; i++) {
    if (!c->p_mask[i] &&
        hipHostMalloc((void **)&c->p_mask[i], (size_t)mask_words(std::max<size_t>(c->max_rows, c->row_cap)) * 8 + 64) != hipSuccess)
      return IBFT_E_NOMEM;
    if (!c->p_tally[i] && hipHostMalloc((void **)&c->p_tally[i], 128) != hipSuccess) return IBFT_E_NOMEM;
    if (!c->dp_mask[i] || !c->dp_tally[i]) {
      void *dm = nullptr, *dt = nullptr;
      if (hipHostGetDevicePointer(&dm, c->p_mask[i], 0) != hipSuccess || hipHostGetDevicePointer(&dt, c->p_tally[i], 0) != hipSuccess)
        return IBFT_E_HIP;
      c->dp_mask[i] = (uint64_t *)dm;
      c->dp_tally[i] = (uint64_t *)dt;
    }
    if (!c->ev_pass[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_pass[i], hipEventDisableTiming));
  }
  return IBFT_OK;
}

// AUTO for the second verdict stream of the pipeline (ibft_seals_submit): only where a side-stream tally may
// follow (no communicator, no local group, key cache off or every table built — never while keys are being learned: both
// learn through one device-wide counter and claim slots), and by default only for the kernel forms the A/B showed a gain for.
static bool alt_verdict_applies(const ibft_ctx *c, uint32_t n) {
  if (c->alt_verdict == 0 || c->side_tally == 0 || n == 0 || c->comm || c->xlocal) return false;
  // (my_built as of the last recount: it only grows until the context's own set changes — a key-cache slot is reused only once
  // no context maps it — so "every table built" still holds when enqueue_recover recounts; d_warm_done exists once and relies on it)
  if (c->cache_on && c->my_built < c->n_validators) return false;
  if (c->alt_verdict == 1) return true;
  // AUTO, measured (profiles/r21_alt_verdict_ab.txt): every warm form, and the cold forms that leave a second workgroup room
  // on a compute unit — two wavefronts / one wavefront / a DPP row per signature, with or without the helper wavefront; NOT
  // the lane / group cold kernels, whose window tables fill the LDS (no side-stream tally behind them either)
  return c->cache_on || cold_lanes_for(c, n) >= 16;
}

// One pipelined pass over the resident batch, its verdict launch on `vs` (the main stream or hstream)
static int seals_submit_on(ibft_ctx *c, hipStream_t vs) {
  const uint32_t s = c->pass_issued & 1u;
  const bool on_alt = vs != c->stream;
  const bool time_it = next_pass_timed(c);
  int rc;
  // The verdict launch writes the CURRENT pair of work mask / validator indices; its last reader was the tally of pass k − 2
  // (collected, or the two-in-flight check of the caller would have refused) or something the main stream is already behind —
  // which hstream has to get behind as well, once, before it carries a verdict launch (main_touched).
  if (on_alt && c->main_touched) {
    for (int i = 0; i < 2; i++)
      if (!c->ev_rec[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_rec[i], hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_rec[s], c->stream));
    HIPCHK(c, hipStreamWaitEvent(vs, c->ev_rec[s], 0));
    c->main_touched = false;
  }
  hipEvent_t after = nullptr;  // right behind this pass's verdict kernels, on vs: the stop event of a timed pass, when it recorded one
  if ((rc = enqueue_recover(c, vs, c->staged_n, c->staged_pre, ibftk::MODE_SEALS, time_it, 0, false, &after))) return rc;
  // Side-stream tally: not for a rank of a sharded batch (its exchange follows the tally on the main stream) and not while
  // keys are still being learned (the tally passes the device's learned-key counter on; with every table built nothing moves it)
  const bool all_warm = c->cache_on && c->my_built >= c->n_validators;
  // AUTO: behind the warm kernels, and behind the cold kernels that leave the tally room (rows / wave / two-wave forms: a quarter
  // of the LDS, a third of the registers) — NOT behind the lane / group kernels whose tables fill the LDS (see side_tally above)
  const bool side = !c->comm && !c->xlocal && (!c->cache_on || all_warm) &&
                    (c->side_tally == 1 || (c->side_tally == 2 && (all_warm || (!c->cache_on && c->last_cold_group >= 16))));
  if (side || on_alt) {
    for (int i = 0; i < 2; i++)
      if (!c->ev_rec[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_rec[i], hipEventDisableTiming));
    if (!after) {  // (an untimed pass, and an empty one: nothing was recorded behind the verdict kernels)
      after = c->ev_rec[s];
      HIPCHK(c, hipEventRecord(after, vs));
    }
  }
  if (side) {
    if (!c->tstream) HIPCHK(c, hipStreamCreateWithFlags(&c->tstream, hipStreamNonBlocking));
    HIPCHK(c, hipStreamWaitEvent(c->tstream, after, 0));
    c->tally_slot = (int)s;
    rc = enqueue_tally(c, c->staged_n, nullptr, c->tstream);
    c->tally_slot = -1;
    if (rc) return rc;
    if (hipEventRecord(c->ev_pass[s], c->tstream) != hipSuccess) {
      // the tally is on its way without an event anybody could wait for: drain its stream before reporting, or the next call on
      // the main stream would share its buffers with it
      (void)hipStreamSynchronize(c->tstream);
      c->last_error = "hipEventRecord behind a side-stream tally failed";
      return IBFT_E_HIP;
    }
    // the next verdict launch gets the other pair; this one belongs to the tally just enqueued until the pass is collected
    std::swap(c->d_mask, c->d_mask_b);
    std::swap(c->d_vidx, c->d_vidx_b);
    std::swap(c->mask_dirty_words, c->mask_dirty_words_b);
    c->side_pending = true;
    c->side_tallies++;
  } else {
    if ((rc = join_side(c))) return rc;   // a main-stream tally shares the sums and verdict words with the side stream's
    if (on_alt) HIPCHK(c, hipStreamWaitEvent(c->stream, after, 0));  // (IBFT_ALT_VERDICT=1 where the side tally does not apply)
    c->main_touched = true;  // this tally reads and zeroes the pair the next verdict launch writes
    c->tally_slot = (int)s;
    rc = enqueue_tally(c, c->staged_n);
    c->tally_slot = -1;
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev_pass[s], c->stream));
  }
  c->pass_n[s] = c->staged_n;
  c->launched_n = c->staged_n;  // (an ibft_seals_fetch behind a submit delivers this pass through the copy route)
  c->pass_issued++;
  c->last_on_alt = on_alt;
  if (on_alt) c->alt_passes++;
  return IBFT_OK;
}

// Pipelined passes over the resident batch: submit enqueues one pass whose results go to one of two host-visible slots,
// collect waits for the OLDEST submitted pass only (the event behind its tally, not the stream).
int ibft_seals_submit(ibft_ctx *c) {
  if (!c) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself: no join_side)
  if (!c->have_valset) return IBFT_E_NOVALSET;
  if (c->pass_issued - c->pass_collected >= 2) {
    c->last_error = "two passes already in flight: call ibft_seals_collect first";
    return IBFT_E_INVAL;
  }
  if (c->bs_issued != c->bs_collected) {  // the two pipelines share the result slots and the spare columns
    c->last_error = "block batches in flight: call ibft_block_seals_collect first";
    return IBFT_E_INVAL;
  }
  if (c->learn_rc != IBFT_OK) {  // the table build behind an already delivered pass failed (ibft_seals_collect): say so once
    const int rc = c->learn_rc;
    c->learn_rc = IBFT_OK;
    return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  {
    const int rcs = ensure_result_slots(c);
    if (rcs) return rcs;
  }
  // consecutive passes alternate between the two verdict streams where that applies (alt_verdict_applies): a pass takes the
  // second one when the pass before it is still in flight and took the main stream
  const bool alt = c->pass_issued != c->pass_collected && !c->last_on_alt && alt_verdict_applies(c, c->staged_n);
  const hipStream_t vs = alt ? c->hstream : c->stream;
  if (alt) c->alt_used = true;
  const int rc = seals_submit_on(c, vs);
  // a failure half way leaves nothing in flight that nobody can wait for: what this call put on hstream (and a tally behind it)
  // has no event a later join could wait for
  if (rc != IBFT_OK && alt) drain_pipeline_streams(c);
  return rc;
}

int ibft_seals_collect(ibft_ctx *c, uint64_t *out_mask, ibft_tally_t *tally) {
  if (!c) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself: no join_side)
  if (c->pass_collected == c->pass_issued) {
    c->last_error = "ibft_seals_collect without a submitted pass";
    return IBFT_E_INVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t s = c->pass_collected & 1u;
  HIPCHK(c, hipEventSynchronize(c->ev_pass[s]));
  const uint64_t *hm = c->p_mask[s], *ht = c->p_tally[s];
  const uint32_t n = c->pass_n[s];
  const size_t mw = (size_t)mask_words(n);
  if (out_mask && mw) {
    memcpy(out_mask, hm, mw * 8);
    if (n & 63) out_mask[mw - 1] &= (~0ull) >> (64 - (n & 63));
  }
  for (int i = 0; i < ibftk::TALLY_SUM_WORDS; i++) c->last_wide[i] = ht[ibftk::TALLY_OUT_WIDE + i];
  if (tally) {
    memset(tally, 0, sizeof *tally);
    tally->quorum_lo = c->quorum_w[0];
    tally->quorum_hi = c->quorum_w[1];
    tally->power_lo = ht[0];
    tally->power_hi = ht[1];
    tally->valid_rows = (uint32_t)(ht[2] & 0xFFFFFFFFull);
    tally->distinct_senders = (uint32_t)(ht[2] >> 32);
    tally->has_quorum = (uint32_t)ht[3];
    tally->proposer_rows = (uint32_t)ht[ibftk::TALLY_OUT_PROPOSER_ROWS];
  }
  // The pass is DELIVERED (its verdict words and tally are in the caller's buffers) before anything else can fail
  // (the count used to move first and a failing table build dropped a finished pass for good).
  c->pass_collected++;
  if (c->cache_on) {  // keys this pass taught the device (passed on by its tally kernel) → tables
    // (build_new_tables waits for the context's whole stream when keys were learned — also for a newer pass in flight:
    // the cold-to-warm transition costs one full drain, include/ibftgpu.h.)  A failure here takes nothing from the verdicts
    // just delivered: the next ibft_seals_submit reports it.
    const uint32_t *lw = reinterpret_cast<const uint32_t *>(ht + 4);
    const int rcb = build_new_tables(c, lw[0], lw[1]);
    if (rcb) c->learn_rc = rcb;
  }
  return IBFT_OK;
}

// Rows of the resident batch and of the oldest submitted pass (0 when none is in flight): a binding sizes its verdict
// buffers from THESE, never from a count its caller passes along (shim/go/ibftgpu).
int ibft_seals_rows(ibft_ctx *c, uint32_t *resident_rows, uint32_t *oldest_pass_rows) {
  if (!c) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself: no join_side)
  if (resident_rows) *resident_rows = c->staged_n;
  if (oldest_pass_rows) *oldest_pass_rows = c->pass_collected == c->pass_issued ? 0u : c->pass_n[c->pass_collected & 1u];
  return IBFT_OK;
}

int ibft_seals_launch(ibft_ctx *c, uint32_t repeat) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  return seals_launch_locked(c, repeat);
}

int ibft_seals_fetch(ibft_ctx *c, uint64_t *out_mask, ibft_tally_t *tally) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  HIPCHK(c, hipSetDevice(c->device));
  return fetch_results(c, c->launched_n, out_mask, tally, true);
}

int ibft_seals_run(ibft_ctx *c, uint64_t *out_mask, ibft_tally_t *tally) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  int rc = seals_launch_locked(c, 1);
  if (rc) return rc;
  return fetch_results(c, c->staged_n, out_mask, tally, true);
}

int ibft_seals_device_ptrs(ibft_ctx *c, void **d_mask, size_t *mask_words_out, void **d_tally) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (d_mask) *d_mask = c->d_mask_out.p;
  if (mask_words_out) *mask_words_out = (size_t)mask_words(c->staged_n);
  if (d_tally) *d_tally = c->d_tally.p;
  return IBFT_OK;
}

int ibft_seals_export(ibft_ctx *c, void *d_mask_dst, void *d_tally_dst) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  HIPCHK(c, hipSetDevice(c->device));
  size_t mw = (size_t)mask_words(c->staged_n);
  if (d_mask_dst && mw)
    HIPCHK(c, hipMemcpyAsync(d_mask_dst, c->d_mask_out.p, mw * 8, hipMemcpyDeviceToDevice, c->stream));
  if (d_tally_dst)
    HIPCHK(c, hipMemcpyAsync(d_tally_dst, c->d_tally.p, 4 * 8, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return IBFT_OK;
}

int ibft_seals_export_on(ibft_ctx *c, void *d_mask_dst, void *d_tally_dst, void *consumer_stream) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t cs = (hipStream_t)consumer_stream;
  {
    int rce = ensure_handoff_events(c);
    if (rce) return rce;
  }
  HIPCHK(c, hipEventRecord(c->ev_ready, c->stream));  // everything launched so far, the tally included
  HIPCHK(c, hipStreamWaitEvent(cs, c->ev_ready, 0));
  size_t mw = (size_t)mask_words(c->staged_n);
  if (d_mask_dst && mw) HIPCHK(c, hipMemcpyAsync(d_mask_dst, c->d_mask_out.p, mw * 8, hipMemcpyDeviceToDevice, cs));
  if (d_tally_dst) HIPCHK(c, hipMemcpyAsync(d_tally_dst, c->d_tally.p, 4 * 8, hipMemcpyDeviceToDevice, cs));
  HIPCHK(c, hipEventRecord(c->ev_read, cs));
  c->read_pending = true;  // enqueue_tally: the next tally overwrites d_mask_out / d_tally only after ev_read
  return IBFT_OK;
}

int ibft_last_kernel_ms(ibft_ctx *c, float *ms, uint32_t *launches) {
  if (!c || !ms) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself: no join_side)
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->alt_used) HIPCHK(c, hipStreamSynchronize(c->hstream));  // (a timed pass's event pair is on the stream that carried it)
  float total = 0.f;
  for (uint32_t i = 0; i < c->ev_used; i++) {
    float t = 0.f;
    HIPCHK(c, hipEventElapsedTime(&t, c->ev[(size_t)i * 2], c->ev[(size_t)i * 2 + 1]));
    total += t;
  }
  *ms = total;
  if (launches) *launches = c->ev_used;
  c->ev_used = 0;
  return IBFT_OK;
}

int ibft_set_kernel_timing(ibft_ctx *c, uint32_t every_n) {
  if (!c) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself: no join_side)
  c->time_every = every_n;
  c->pass_counter = 0;
  return IBFT_OK;
}

int ibft_cache_stats(ibft_ctx *c, uint32_t *tables, uint32_t *warm_passes, uint32_t *cold_passes,
                     uint32_t *lanes_per_signature) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (tables) *tables = c->cache_on ? c->my_built : 0;
  if (warm_passes) *warm_passes = c->warm_passes;
  if (cold_passes) *cold_passes = c->cold_passes;
  if (lanes_per_signature) *lanes_per_signature = c->last_group;
  return IBFT_OK;
}

int ibft_cache_memory(ibft_ctx *c, uint64_t *device_bytes, uint32_t *slots_in_use, uint32_t *slots_allocated,
                      uint32_t *contexts_sharing) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  std::lock_guard<std::mutex> dlk(c->dev->mu);
  const DeviceShared &d = *c->dev;
  if (device_bytes) *device_bytes = (uint64_t)d.d_gtab.cap + d.d_qtab.cap + d.d_pub.cap + d.d_state.cap + d.d_learned.cap;
  if (slots_in_use) *slots_in_use = d.used - (uint32_t)d.free_slots.size();
  if (slots_allocated) *slots_allocated = d.cap;
  if (contexts_sharing) *contexts_sharing = (uint32_t)c->dev.use_count();
  return IBFT_OK;
}

int ibft_cache_form(ibft_ctx *c, uint32_t *form, uint64_t *slot_bytes) {
  if (!c) return IBFT_E_INVAL;
  // (set when the device's shared object was created, never changed: no lock)
  if (form) *form = (uint32_t)c->dev->form;
  if (slot_bytes) *slot_bytes = (uint64_t)c->dev->slot_bytes;
  return IBFT_OK;
}

int ibft_last_dispatch(ibft_ctx *c, uint32_t *cold_lanes, uint32_t *warm_lanes) {
  if (!c) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself: no join_side)
  if (cold_lanes) *cold_lanes = c->last_cold_group;
  if (warm_lanes) *warm_lanes = c->last_group;
  return IBFT_OK;
}

int ibft_last_cold_table(ibft_ctx *c, uint32_t *table) {
  if (!c || !table) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself: no join_side)
  *table = (c->last_cold_group == 1 || c->last_cold_group == 2 || c->last_cold_group == 4) ? c->last_cold_table : 0u;
  return IBFT_OK;
}

int ibft_pipeline_stats(ibft_ctx *c, uint32_t *side_tallies, uint32_t *split_batches) {
  if (!c) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself: no join_side)
  if (side_tallies) *side_tallies = c->side_tallies;
  if (split_batches) *split_batches = c->split_launches;
  return IBFT_OK;
}

int ibft_pipeline_stats_ex(ibft_ctx *c, uint32_t *side_tallies, uint32_t *split_batches, uint32_t *alt_verdicts) {
  if (!c) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself: no join_side)
  if (side_tallies) *side_tallies = c->side_tallies;
  if (split_batches) *split_batches = c->split_launches;
  if (alt_verdicts) *alt_verdicts = c->alt_passes;
  return IBFT_OK;
}

int ibft_column_stats(ibft_ctx *c, uint32_t *gather_batches) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (gather_batches) *gather_batches = c->gathers;
  return IBFT_OK;
}

void *ibft_pinned_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) return nullptr;
  void *dp = nullptr;
  // the gather launch dereferences the host address itself: only register blocks the device sees at that address
  if (hipHostGetDevicePointer(&dp, p, 0) == hipSuccess && dp == p) {
    std::lock_guard<std::mutex> lk(pinned_registry().mu);
    pinned_registry().blocks[(uintptr_t)p] = bytes ? bytes : 1;
  }
  return p;
}
void ibft_pinned_free(void *p) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> lk(pinned_registry().mu);
    pinned_registry().blocks.erase((uintptr_t)p);
  }
  (void)hipHostFree(p);
}

// ---- What the two message-set routes share (columns: messages_launch_locked + ibft_verify_messages; wire bytes:
// ibft_verify_messages_wire): the proposal in front, the combine step and tally behind the verdict launch, the two endings.
// c->mu held throughout.

// The proposal the set is checked against: the caller's digest, or raw ‖ BE64(round) hashed once and remembered.
// *hash_needed: that hash is still to be launched (enqueue_set_tally does; an empty set's caller does it itself)
static int set_proposal_begin(ibft_ctx *c, const uint8_t *digest32, const uint8_t *raw, size_t raw_len, uint64_t round, bool *hash_needed) {
  *hash_needed = false;
  if (!digest32) {
    *hash_needed = note_proposal(c, raw, raw_len, round);
    return IBFT_OK;
  }
  int rc;
  if ((rc = wait_proposal_hash(c))) return rc;  // a hash still on its way must not land on top of the caller's digest
  c->have_H = false;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging buffer is free again
  memcpy(c->h_digest, digest32, 32);
  HIPCHK(c, hipMemcpyAsync(c->d_H.p, c->h_digest, 32, hipMemcpyHostToDevice, c->stream));
  return IBFT_OK;
}

// what the combine step of a set is told beyond the columns both routes share (device pointers; null / 0 / false: absent)
struct set_tail {
  const uint8_t *sender_pre = nullptr, *valid_pre = nullptr;  // rows rejected before any crypto, per verdict
  const uint8_t *no_seal = nullptr;                           // rows whose closure has no seal (PREPAREs among wire rows)
  uint32_t half_words = 0;     // where the seal rows' verdict words begin (0: no seal half)
  bool converted = false;      // a1 compares the carried hashes apply_seal_digest kept in d_hash_copy
  bool hash_needed = false;    // set_proposal_begin's answer
  // the wire call notes its proposer HERE, behind the hash wait: a failure in front of it leaves none to a later call
  bool note_proposer = false;
  const uint8_t *proposer20 = nullptr;
};
// Behind the verdict launch of a set of n rows whose carried hashes are rows [half, half + n) of the hash column: the
// proposal's hash (launched on the side stream if still needed, waited for), the combine step and tally, the words' way home.
static int enqueue_set_tally(ibft_ctx *c, size_t n, uint32_t half, const set_tail &t) {
  int rc;
  ibftk::set_args sa{};
  sa.sender_pre = t.sender_pre;
  sa.valid_pre = t.valid_pre;
  sa.no_seal = t.no_seal;
  sa.hash32 = t.converted ? (const uint8_t *)c->d_hash_copy.p : (const uint8_t *)c->d_hash.p + 32ull * half;
  sa.hash_len = (const uint8_t *)c->d_hash_len.p;
  sa.H4 = (const uint64_t *)c->d_H.p;
  sa.n = (uint32_t)n;
  sa.half_words = t.half_words;
  sa.sender_out = (uint64_t *)c->d_set.p;
  sa.valid_out = (uint64_t *)c->d_set.p + mask_words(c->max_rows);
  sa.host_sender = c->dh_set;
  sa.host_valid = c->dh_set ? c->dh_set + mask_words(c->max_rows) : nullptr;
  // the verdict launch did not need the proposal's hash, the combine step does: hashed on the side stream meanwhile
  if (t.hash_needed && (rc = launch_proposal_hash(c))) return rc;
  if ((rc = wait_proposal_hash(c))) return rc;
  if (t.note_proposer) note_proposer(c, t.proposer20);
  if ((rc = enqueue_tally(c, (uint32_t)n, &sa))) return rc;
  // the combine step zeroed the seal words, the tally the sender words (the lane kernel stores whole words and asks for no
  // clean mask in front)
  mask_consumed(c, mask_words(t.half_words ? (size_t)half + n : n));
  if (!c->dh_set)
    HIPCHK(c, hipMemcpyAsync(c->h_set, c->d_set.p, (size_t)mask_words(c->max_rows) * 16, hipMemcpyDeviceToHost, c->stream));
  return IBFT_OK;
}

// The answer to a set without rows.  With a proposer, HasPrepareQuorum of no messages is still a question (the proposer alone
// may be a quorum: validator_manager.go:109-126) and the tally the caller enqueued answers it; without one, a zero tally.
static int answer_empty_set(ibft_ctx *c, const uint8_t *proposer20, ibft_tally_t *tally) {
  if (proposer20) return fetch_results(c, 0, nullptr, tally, true);
  if (tally) {
    memset(tally, 0, sizeof *tally);
    tally->quorum_lo = c->quorum_w[0];
    tally->quorum_hi = c->quorum_w[1];
  }
  for (int i = 0; i < ibftk::TALLY_SUM_WORDS; i++) c->last_wide[i] = 0;
  return IBFT_OK;
}

// … and to one with rows: the tally, then the sender and the valid words out of h_set
static int fetch_set_masks(ibft_ctx *c, size_t n, uint64_t *out_sender_mask, uint64_t *out_valid_mask, ibft_tally_t *tally) {
  int rc;
  if ((rc = fetch_results(c, (uint32_t)n, nullptr, tally, true))) {
    c->have_H = false;
    return rc;
  }
  const size_t mw = (size_t)mask_words(n);
  memcpy(out_sender_mask, c->h_set, mw * 8);
  memcpy(out_valid_mask, c->h_set + mask_words(c->max_rows), mw * 8);
  return IBFT_OK;
}

// A whole PREPARE or COMMIT set in one call (kernels.hip.h: "a message set in one pass").
// a message set up to and including its tally, everything asynchronous past the uploads (c->mu held)
static int messages_launch_locked(ibft_ctx *c, const uint8_t *payload, const uint32_t *off, const uint8_t *msg_sig65,
                                  const uint8_t *from20, const uint8_t *hash32, const uint8_t *hash_len, const uint8_t *seal65,
                                  const uint8_t *sender_pre, const uint8_t *valid_pre, size_t n, const uint8_t *raw, size_t raw_len,
                                  uint64_t round, const uint8_t *digest32) {
  if (n && (!off || !msg_sig65 || !from20 || !hash32 || !hash_len)) return IBFT_E_INVAL;
  if ((raw_len && !raw) || raw_len > (1ull << 31)) return IBFT_E_INVAL;
  if (!offsets_ok(off, n) || !bytes_ok(off, n, payload)) return IBFT_E_INVAL;
  if (n > c->max_rows) return IBFT_E_TOOBIG;
  if (!c->have_valset) return IBFT_E_NOVALSET;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  c->wire.columns = false;
  c->staged_n = 0;
  c->set_n = (uint32_t)n;
  const uint32_t half = ((uint32_t)n + 63u) & ~63u;
  const uint32_t rows = seal65 ? half + (uint32_t)n : (uint32_t)n;  // verdict rows of the one launch
  if ((rc = alloc_rows(c, 2 * (((uint32_t)c->max_rows + 63u) & ~63u)))) return rc;
  bool hash_needed;
  if ((rc = set_proposal_begin(c, digest32, raw, raw_len, round, &hash_needed))) return rc;
  if (n == 0) {
    if (hash_needed && (rc = launch_proposal_hash(c))) return rc;
    // an empty shard of a sharded set still contributes (zero) words, an empty bitmap and a zero count to the exchange;
    // so does the set of a caller that noted a proposer (answer_empty_set)
    if (c->comm || c->xlocal || c->next_prop_on) return enqueue_tally(c, 0);
    return IBFT_OK;
  }
  uint8_t *d_hash = (uint8_t *)c->d_hash.p, *d_sig = (uint8_t *)c->d_sig.p, *d_signer = (uint8_t *)c->d_signer.p,
          *d_pre = (uint8_t *)c->d_pre.p;
  const size_t pbytes = off[n];
  if ((rc = ensure(c, c->d_payload, pbytes + 256))) return rc;
  ColumnCopies cc;
  cc.payload(c->d_payload.p, payload, pbytes, c->d_off.p, off, n, d_hash);
  cc.add(d_sig, msg_sig65, n * 65);
  cc.add(d_signer, from20, n * 20);
  cc.add(d_hash + 32ull * half, hash32, n * 32);  // the hashes the messages carry
  cc.add(c->d_hash_len.p, hash_len, n);
  // rows the host rejected before any crypto: applied to the verdict words afterwards (the verdict launch runs them
  // like any other row — skipping work inside a lock-step wavefront saves nothing)
  if (sender_pre) cc.add(d_pre, sender_pre, n);
  if (valid_pre) cc.add(d_pre + half, valid_pre, n);
  if (seal65) {
    cc.add(d_sig + 65ull * half, seal65, n * 65);
    cc.add(d_signer + 20ull * half, from20, n * 20);  // the seal's signer is the message's From
    if (half != n)  // rows n..half−1 sit between the two groups: a zero signature is rejected by every kernel
      HIPCHK(c, hipMemsetAsync(d_sig + 65ull * n, 0, 65ull * (half - n), c->stream));
  }
  if ((rc = cc.flush(c))) return rc;
  if (!cc.digest_done) {  // pageable columns: the payload was copied, hash it from HBM
    hipLaunchKernelGGL(ibftk::payload_digest_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream,
                       (const uint8_t *)c->d_payload.p, (const uint32_t *)c->d_off.p, (uint32_t)n, d_hash);
    HIPCHK(c, hipGetLastError());
  }
  // the seals sign digest(carried hash) under a non-identity convention; a1 still compares the carried hashes (the copy)
  const bool converted = seal65 && c->seal_digest_mode != 0;
  if (converted && (rc = apply_seal_digest(c, (uint8_t *)c->d_hash.p + 32ull * half, (uint32_t)n, true))) return rc;
  c->ev_used = 0;
  const bool time_it = c->time_every && (c->pass_counter++ % c->time_every) == 0;
  if ((rc = enqueue_recover(c, c->stream, rows, /*with_pre=*/false, ibftk::MODE_SEALS, time_it))) return rc;
  set_tail t;
  t.sender_pre = sender_pre ? d_pre : nullptr;
  t.valid_pre = valid_pre ? d_pre + half : nullptr;
  t.half_words = seal65 ? half / 64 : 0;
  t.converted = converted;
  t.hash_needed = hash_needed;
  return enqueue_set_tally(c, n, half, t);  // (the proposer, if any, was noted by the caller)
}

int ibft_verify_messages(ibft_ctx *c, const uint8_t *payload, const uint32_t *off, const uint8_t *msg_sig65,
                         const uint8_t *from20, const uint8_t *hash32, const uint8_t *hash_len, const uint8_t *seal65,
                         const uint8_t *sender_pre, const uint8_t *valid_pre, size_t n, const uint8_t *raw, size_t raw_len,
                         uint64_t round,
                         const uint8_t *digest32, const uint8_t *proposer20, uint64_t *out_sender_mask,
                         uint64_t *out_valid_mask, ibft_tally_t *tally) {
  if (!c || (n && (!out_sender_mask || !out_valid_mask))) return IBFT_E_INVAL;
  ctx_lock lk(c);
  note_proposer(c, proposer20);
  int rc = messages_launch_locked(c, payload, off, msg_sig65, from20, hash32, hash_len, seal65, sender_pre, valid_pre, n, raw,
                                  raw_len, round, digest32);
  c->next_prop_on = c->next_shard = false;  // (an error in front of the tally must not leave the proposer to a later call)
  if (rc) return rc;
  if (n == 0) return answer_empty_set(c, proposer20, tally);  // (its tally: messages_launch_locked, the proposer being noted)
  return fetch_set_masks(c, n, out_sender_mask, out_valid_mask, tally);
}

// f4: the committed seals of a simulated validator set, one per row.
int ibft_sign_seals(ibft_ctx *c, const uint8_t *sk32, const uint8_t *hash32, size_t n, uint8_t *out_sig65,
                    uint8_t *out_signer20, uint8_t *out_ok) {
  return ibft_sign_seals_ex(c, sk32, hash32, n, IBFT_SIGN_NONCE_KECCAK, out_sig65, out_signer20, out_ok);
}

// the same under a chosen nonce rule: one instantiation of sign_lane_kernel per rule
int ibft_sign_seals_ex(ibft_ctx *c, const uint8_t *sk32, const uint8_t *hash32, size_t n, uint32_t nonce, uint8_t *out_sig65,
                       uint8_t *out_signer20, uint8_t *out_ok) {
  if (!c || (n && (!sk32 || !hash32 || !out_sig65))) return IBFT_E_INVAL;
  ctx_lock lk(c);
  sign_call sc{c, nonce, n};
  int rc;
  if ((rc = sc.check("ibft_sign_seals_ex")) || (rc = sc.begin())) return rc;
  if (n == 0) return IBFT_OK;
  if ((rc = sc.upload_keys(sk32)) || (rc = upload(c, c->d_hash, hash32, n * 32))) return rc;
  if ((rc = apply_seal_digest(c, c->d_hash.p, (uint32_t)n))) return rc;  // a seal signs what the convention says it signs
  ibftk::sign_args a;
  a.gtab = (const uint32_t *)c->dev->d_gtab.p;
  a.sk32 = (const uint8_t *)c->d_payload.p;
  a.hash32 = (const uint8_t *)c->d_hash.p;
  a.sig65 = (uint8_t *)c->d_sig.p;
  a.signer20 = (uint8_t *)c->d_signer.p;
  a.ok = (uint8_t *)c->d_pre.p;
  a.n = (uint32_t)n;
  sc.launch_signed([](auto N) { return ibftk::sign_lane_kernel<decltype(N)::value>; }, a);
  if ((rc = sc.finish(out_sig65, c->d_sig.p, n * 65, out_signer20, out_ok))) return rc;
  // hash32 / sig65 / signer20 now hold exactly what ibft_seals_stage would have uploaded for these seals:
  // the batch is staged (rows whose key was refused carry a zero signature, which every verifier rejects)
  c->staged_n = (uint32_t)n;
  c->staged_pre = false;
  return IBFT_OK;
}

// f4 one layer up: whole PREPARE / COMMIT messages as wire bytes (sign_message_dev.h).  A row's length depends on type, height
// and round alone, so the offsets are computed here, before anything is launched, and uploaded.
int ibft_sign_messages_wire(ibft_ctx *c, const uint8_t *sk32, const uint8_t *type, const uint64_t *height, const uint64_t *round,
                            const uint8_t *hash32, size_t n, uint32_t nonce, uint8_t *out_wire, size_t wire_cap, uint32_t *out_off,
                            uint8_t *out_from20, uint8_t *out_ok) {
  if (!c || (n && (!sk32 || !type || !height || !round || !hash32 || !out_wire || !out_off))) return IBFT_E_INVAL;
  ctx_lock lk(c);
  sign_call sc{c, nonce, n};
  int rc;
  if ((rc = sc.check("ibft_sign_messages_wire"))) return rc;
  std::vector<uint32_t> off(n + 1);
  uint64_t total = 0;
  for (size_t i = 0; i < n; i++) {
    if (type[i] != ibftk::MSG_TYPE_PREPARE && type[i] != ibftk::MSG_TYPE_COMMIT) {
      c->last_error = "ibft_sign_messages_wire: row " + std::to_string(i) + " has type " + std::to_string((unsigned)type[i]) +
                      " (1 = PREPARE, 2 = COMMIT)";
      return IBFT_E_INVAL;
    }
    off[i] = (uint32_t)total;
    total += ibftk::message_wire_len(type[i], height[i], round[i]);
  }
  off[n] = (uint32_t)total;
  if (total > wire_cap || total > 0xFFFFFFFFull) {
    c->last_error = "ibft_sign_messages_wire: the messages take " + std::to_string(total) + " bytes, wire_cap is " + std::to_string(wire_cap);
    return IBFT_E_TOOBIG;
  }
  if ((rc = sc.begin())) return rc;
  if (n == 0) {
    if (out_off) out_off[0] = 0;
    return IBFT_OK;
  }
  const size_t col = (n + 7) & ~(size_t)7;  // the type bytes sit behind two 8-byte columns
  if ((rc = ensure(c, c->d_msg_cols, 17 * col))) return rc;
  if ((rc = ensure(c, c->d_msg_wire, (size_t)total))) return rc;
  uint8_t *cols = (uint8_t *)c->d_msg_cols.p;
  HIPCHK(c, hipMemcpyAsync(cols, height, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(cols + 8 * col, round, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(cols + 16 * col, type, n, hipMemcpyHostToDevice, c->stream));
  if ((rc = sc.upload_keys(sk32)) || (rc = upload(c, c->d_hash, hash32, n * 32))) return rc;
  if ((rc = upload(c, c->d_off, off.data(), (n + 1) * 4))) return rc;
  ibftk::sign_message_args a;
  a.gtab = (const uint32_t *)c->dev->d_gtab.p;
  a.sk32 = (const uint8_t *)c->d_payload.p;
  a.type = cols + 16 * col;
  a.height = (const uint64_t *)cols;
  a.round = (const uint64_t *)(cols + 8 * col);
  a.hash32 = (const uint8_t *)c->d_hash.p;
  a.off = (const uint32_t *)c->d_off.p;
  a.wire = (uint8_t *)c->d_msg_wire.p;
  a.from20 = (uint8_t *)c->d_signer.p;
  a.ok = (uint8_t *)c->d_pre.p;
  a.n = (uint32_t)n;
  a.convert = c->seal_digest_mode != 0 ? 1u : 0u;  // the seal signs what the convention says it signs; the envelope never does
  memcpy(a.suffix_words, c->seal_suffix_words, sizeof a.suffix_words);
  sc.launch_signed([](auto N) { return ibftk::sign_message_lane_kernel<decltype(N)::value>; }, a);
  if ((rc = sc.finish(out_wire, c->d_msg_wire.p, (size_t)total, out_from20, out_ok))) return rc;
  memcpy(out_off, off.data(), (n + 1) * 4);
  return IBFT_OK;
}

// f4 two layers up: PREPREPARE / ROUND_CHANGE envelopes around bodies the caller encoded (sign_envelope_dev.h).  A row's length
// depends on type, height, round and body length alone, so offsets, body destinations and the copy kernel's pieces are computed
// here, in one pass, before anything is launched.  Four launches on the main stream: heads, body copy, digests, signatures.
int ibft_sign_envelopes_wire(ibft_ctx *c, const uint8_t *sk32, const uint8_t *type, const uint64_t *height, const uint64_t *round,
                             const uint8_t *body, size_t body_bytes, const uint32_t *body_at, const uint32_t *body_len, size_t n,
                             uint32_t nonce, uint8_t *out_wire, size_t wire_cap, uint32_t *out_off, uint8_t *out_from20, uint8_t *out_ok) {
  if (!c || (n && (!sk32 || !type || !height || !round || !body_at || !body_len || !out_wire || !out_off))) return IBFT_E_INVAL;
  if (!body && body_bytes) return IBFT_E_INVAL;
  ctx_lock lk(c);
  sign_call sc{c, nonce, n};
  int rc;
  if ((rc = sc.check("ibft_sign_envelopes_wire"))) return rc;
  for (size_t i = 0; i < n; i++) {
    if (type[i] != ibftk::MSG_TYPE_PREPREPARE && type[i] != ibftk::MSG_TYPE_ROUND_CHANGE) {
      c->last_error = "ibft_sign_envelopes_wire: row " + std::to_string(i) + " has type " + std::to_string((unsigned)type[i]) +
                      " (0 = PREPREPARE, 3 = ROUND_CHANGE)";
      return IBFT_E_INVAL;
    }
  }
  for (size_t i = 0; i < n; i++) {
    if ((uint64_t)body_at[i] + body_len[i] > body_bytes) {  // (64-bit: at + len may pass 2^32)
      c->last_error = "ibft_sign_envelopes_wire: row " + std::to_string(i) + " names body bytes [" + std::to_string(body_at[i]) + ", " +
                      std::to_string((uint64_t)body_at[i] + body_len[i]) + ") of " + std::to_string(body_bytes);
      return IBFT_E_INVAL;
    }
  }
  // host columns, one upload: height ‖ round (8-byte entries) ‖ body_at ‖ body_len ‖ dst_at ‖ off[n+1] ‖ piece_first[n+1] ‖ type
  const size_t col = (n + 8) & ~(size_t)7;  // entries per column, room for the n + 1 of the last two
  std::vector<uint64_t> cols((16 * col + 20 * col + col + 7) / 8);
  uint8_t *h = (uint8_t *)cols.data();
  uint64_t *h_height = (uint64_t *)h, *h_round = h_height + col;
  uint32_t *h_at = (uint32_t *)(h + 16 * col), *h_len = h_at + col, *h_dst = h_len + col, *h_off = h_dst + col, *h_piece = h_off + col;
  uint8_t *h_type = h + 36 * col;
  uint64_t total = 0, total_blocks = 0, max_blocks = 0, pieces = 0;
  for (size_t i = 0; i < n; i++) {  // (dst_at, off and piece_first in front of the size checks, which read this pass's totals)
    const uint32_t head = ibftk::envelope_head_len(type[i], height[i], round[i], body_len[i]);
    const uint64_t blocks = ((uint64_t)head + body_len[i] - ibftk::SIGN_MESSAGE_SIG_FIELD) / 136u + 1u;
    h_off[i] = (uint32_t)total;
    h_dst[i] = (uint32_t)total + head;
    h_piece[i] = (uint32_t)pieces;
    pieces += ibftk::envelope_copy_pieces(h_dst[i], body_len[i]);  // (≤ total / 4 096 + 2 n in all)
    total += (uint64_t)head + body_len[i];                         // (n ≤ max_rows rows of < 2^33 bytes: no overflow)
    total_blocks += blocks;
    max_blocks = std::max(max_blocks, blocks);
  }
  if (body_bytes > c->proposal_bytes_max || total > c->proposal_bytes_max) {
    c->last_error = "ibft_sign_envelopes_wire: " + std::to_string(body_bytes) + " body bytes in, " + std::to_string(total) +
                    " bytes out: more than the proposal byte budget of " + std::to_string(c->proposal_bytes_max) + " (IBFT_PROPOSAL_BYTES_MAX)";
    return IBFT_E_TOOBIG;
  }
  if (total > wire_cap) {
    c->last_error = "ibft_sign_envelopes_wire: the messages take " + std::to_string(total) + " bytes, wire_cap is " + std::to_string(wire_cap);
    return IBFT_E_TOOBIG;
  }
  if ((rc = sc.begin())) return rc;
  if (n == 0) {
    if (out_off) out_off[0] = 0;
    return IBFT_OK;
  }
  h_off[n] = (uint32_t)total;
  h_piece[n] = (uint32_t)pieces;
  memcpy(h_height, height, n * 8);
  memcpy(h_round, round, n * 8);
  memcpy(h_at, body_at, n * 4);
  memcpy(h_len, body_len, n * 4);
  memcpy(h_type, type, n);
  if ((rc = ensure(c, c->d_env_body, body_bytes + 256))) return rc;  // the copy and the sponges read a few bytes past a range
  if ((rc = ensure(c, c->d_env_wire, (size_t)total + 256))) return rc;
  if ((rc = ensure(c, c->d_hash, n * 32))) return rc;
  if ((rc = upload(c, c->d_env_cols, h, 37 * col))) return rc;
  if (body_bytes) HIPCHK(c, hipMemcpyAsync(c->d_env_body.p, body, body_bytes, hipMemcpyHostToDevice, c->stream));
  if ((rc = sc.upload_keys(sk32))) return rc;
  const uint8_t *d = (const uint8_t *)c->d_env_cols.p;
  ibftk::sign_envelope_args a;
  a.gtab = (const uint32_t *)c->dev->d_gtab.p;
  a.sk32 = (const uint8_t *)c->d_payload.p;
  a.type = d + 36 * col;
  a.height = (const uint64_t *)d;
  a.round = (const uint64_t *)(d + 8 * col);
  a.body = (const uint8_t *)c->d_env_body.p;
  a.body_at = (const uint32_t *)(d + 16 * col);
  a.body_len = a.body_at + col;
  a.dst_at = a.body_len + col;
  a.off = a.dst_at + col;
  a.piece_first = a.off + col;
  a.wire = (uint8_t *)c->d_env_wire.p;
  a.digest32 = (uint8_t *)c->d_hash.p;
  a.from20 = (uint8_t *)c->d_signer.p;
  a.ok = (uint8_t *)c->d_pre.p;
  a.n = (uint32_t)n;
  hipLaunchKernelGGL(ibftk::envelope_head_kernel, dim3(sc.blocks()), dim3(ibftk::ROWS_PER_BLOCK), 0, c->stream, a);
  if (pieces) hipLaunchKernelGGL(ibftk::envelope_copy_kernel, dim3((uint32_t)pieces), dim3(ibftk::ENVELOPE_COPY_THREADS), 0, c->stream, a);
  // the digest's form by proposal_form's rule: the batch's size in messages of the longest one's length
  const uint32_t form = c->envelope_lanes_force ? c->envelope_lanes_force
                        : (n >= 64 && total_blocks >= (uint64_t)c->proposal_lane_rows * max_blocks) ? 1u : 64u;
  if (form == 1)
    hipLaunchKernelGGL(ibftk::envelope_digest_kernel<1>, dim3(sc.blocks()), dim3(64), 0, c->stream, a);
  else
    hipLaunchKernelGGL(ibftk::envelope_digest_kernel<64>, dim3((uint32_t)n), dim3(64), 0, c->stream, a);
  sc.launch_signed([](auto N) { return ibftk::sign_envelope_lane_kernel<decltype(N)::value>; }, a);
  if ((rc = sc.finish(out_wire, c->d_env_wire.p, (size_t)total, out_from20, out_ok))) return rc;
  memcpy(out_off, h_off, (n + 1) * 4);
  return IBFT_OK;
}

// Device canary: see issue_probe_kernel (kernels.hip.h).  Three untimed launches, then the median of five timed ones.
int ibft_issue_probe(ibft_ctx *c, float *ns_per_inst, float *kernel_ms) {
  if (!c || !ns_per_inst) return IBFT_E_INVAL;
  ctx_lock lk(c);
  HIPCHK(c, hipSetDevice(c->device));
  uint32_t *d_out = nullptr;
  HIPCHK(c, hipMalloc(&d_out, 64));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = IBFT_OK;
  float t[5] = {0, 0, 0, 0, 0};
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = IBFT_E_HIP;
  for (int k = 0; k < 8 && rc == IBFT_OK; k++) {
    if (k >= 3 && hipEventRecord(e0, c->stream) != hipSuccess) rc = IBFT_E_HIP;
    hipLaunchKernelGGL(ibftk::issue_probe_kernel, dim3(256), dim3(256), 0, c->stream, d_out, (uint32_t)(k + 1));
    if (k >= 3) {
      if (hipEventRecord(e1, c->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
          hipEventElapsedTime(&t[k - 3], e0, e1) != hipSuccess)
        rc = IBFT_E_HIP;
    }
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess) rc = IBFT_E_HIP;
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(d_out);
  if (rc != IBFT_OK) {
    c->last_error = "ibft_issue_probe: a HIP call failed";
    return rc;
  }
  std::sort(t, t + 5);
  if (kernel_ms) *kernel_ms = t[2];
  *ns_per_inst = t[2] * 1e6f / (float)(ibftk::ISSUE_PROBE_ITERS * 64);
  return IBFT_OK;
}

int ibft_sync(ibft_ctx *c) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->alt_used) HIPCHK(c, hipStreamSynchronize(c->hstream));  // (the main stream is behind it already: ctx_lock → join_side)
  if (c->xstream) HIPCHK(c, hipStreamSynchronize(c->xstream));  // exchanges in flight (ibft_seals_exchange)
  if (c->cstream) HIPCHK(c, hipStreamSynchronize(c->cstream));  // a batch on its way into the spare slot (ibft_seals_stage_next)
  if (c->ostream) HIPCHK(c, hipStreamSynchronize(c->ostream));  // digests / emitted columns of streamed block batches on their way out
  return IBFT_OK;
}

int ibft_verify_seals(ibft_ctx *c, const uint8_t *hash32, const uint8_t *sig65, const uint8_t *signer20,
                      const uint8_t *pre_flags, size_t n, uint64_t *out_mask, ibft_tally_t *tally) {
  if (!c || (n && !out_mask)) return IBFT_E_INVAL;
  ctx_lock lk(c);  // one critical section: stage + launch + fetch
  if (!c->have_valset) return IBFT_E_NOVALSET;
  int rc;
  if ((rc = seals_stage_locked(c, hash32, sig65, signer20, pre_flags, n, false))) return rc;
  if ((rc = seals_launch_locked(c, 1))) return rc;
  return fetch_results(c, c->staged_n, out_mask, tally, true);
}

// The emitted columns of the last MODE_EMIT launch → the caller's buffers, on the main stream (behind the tally, which only
// reads the validator indices).  The caller synchronises.
static int copy_emitted(ibft_ctx *c, size_t n, uint8_t *out_signer20, int32_t *out_vidx) {
  if (!n) return IBFT_OK;
  HIPCHK(c, hipMemcpyAsync(out_signer20, c->d_signer_out.p, n * 20, hipMemcpyDeviceToHost, c->stream));
  if (out_vidx) HIPCHK(c, hipMemcpyAsync(out_vidx, c->d_vidx.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  return IBFT_OK;
}

// Bare seals: who signed?  The cold kernels in their emitting form, then the tally over the validator indices they found.
int ibft_recover_seals(ibft_ctx *c, const uint8_t *hash32, const uint8_t *sig65, const uint8_t *pre_flags, size_t n,
                       uint8_t *out_signer20, int32_t *out_vidx, uint64_t *out_mask, ibft_tally_t *tally) {
  if (!c || (n && (!out_signer20 || !out_mask))) return IBFT_E_INVAL;
  ctx_lock lk(c);  // one critical section: stage + launch + fetch
  if (!c->have_valset) return IBFT_E_NOVALSET;
  int rc;
  if ((rc = seals_stage_locked(c, hash32, sig65, nullptr, pre_flags, n, false, true))) return rc;
  if ((rc = seals_launch_locked(c, 1, ibftk::MODE_EMIT))) return rc;
  if ((rc = copy_emitted(c, n, out_signer20, out_vidx))) return rc;
  rc = fetch_results(c, (uint32_t)n, out_mask, tally, true);
  c->staged_n = 0;  // bare rows are no resident batch: there is no signer column ibft_seals_launch could judge them against
  return rc;
}

// The segmented tally of a block batch over the resident work mask / validator indices and the offsets in d_boff, on the main
// stream.  Work mask, the bitmap and the ticket word in d_acc exist once per context: two batches in flight
// (ibft_block_seals_submit) take turns at them in main-stream order.  sets: under a family of validator sets (the block's set
// in d_block_set: fam.d_bset, or the column of a streamed batch's slot) — powers, quorums and bitmap are the family's, the
// LARGEST set in the place of the one set's size.  fam.d_seen exists once: sets tallies stay on the MAIN stream, where two
// batches in flight take turns at it; the side-tally rule of the seal pipeline (enqueue_tally's `on`) does not apply to them.
static int enqueue_block_tally(ibft_ctx *c, uint32_t nb, uint32_t nr, uint32_t widest, uint64_t *host_mask, uint64_t *out, bool sets,
                               const void *d_block_set = nullptr) {
  int rc;
  if ((rc = wait_for_readers(c, c->stream))) return rc;
  const ValFamily &f = c->fam;
  ibftk::block_tally_sets_args t{};
  t.work_mask = (uint64_t *)c->d_mask.p;
  t.mask = (uint64_t *)c->d_mask_out.p;
  t.host_mask = host_mask;
  t.vidx = (int32_t *)c->d_vidx.p;
  t.vpower32 = (const uint32_t *)(sets ? f.d_power.p : c->d_vpower.p);
  t.off = (const uint32_t *)c->d_boff.p;
  t.n = nr;
  t.n_blocks = nb;
  t.n_validators = c->n_validators;  // (under family_view: the union's size)
  size_t dyn;
  t.lds_bitmap = bitmap_in_lds(sets ? f.largest_set : c->n_validators, &dyn);  // 0: one workgroup walks every block over the HBM bitmap
  t.seen = (uint32_t *)(sets ? f.d_seen.p : c->d_seen.p);
  t.acc = (uint64_t *)c->d_acc.p;
  t.quorum = (const uint64_t *)(sets ? f.d_quorum.p : c->d_quorum.p);
  t.out = out;
  t.block_set = (const uint32_t *)(d_block_set ? d_block_set : f.d_bset.p);  // (these three: read by the sets form alone)
  t.setidx = (const int32_t *)f.d_setidx.p;
  t.set_meta = (const uint2 *)f.d_meta.p;
  const dim3 grid(t.lds_bitmap ? std::min(nb, ibftk::BTALLY_MAX_GRID) : 1u);
  const bool wide = widest > 256u * ibftk::BTALLY_RPT;  // a block that one step of 256 threads does not cover
  const ibftk::block_tally_args &plain = t;
  with_power_words(sets ? f.power_words : c->power_words, [&](auto PW) {
    with_int<1024, 256>(wide ? 1024 : 256, [&](auto THREADS) {
      if (sets) hipLaunchKernelGGL((ibftk::block_tally_kernel<decltype(PW)::value, decltype(THREADS)::value, true>), grid, dim3(decltype(THREADS)::value), dyn, c->stream, t);
      else hipLaunchKernelGGL((ibftk::block_tally_kernel<decltype(PW)::value, decltype(THREADS)::value, false>), grid, dim3(decltype(THREADS)::value), dyn, c->stream, plain);
    });
  });
  HIPCHK(c, hipGetLastError());
  mask_consumed(c, mask_words(nr));
  return IBFT_OK;
}

// ---- chain sync from the proposals: keccak256(RawProposal ‖ BE64(Round)) of n proposals on the device ------------------------
// A batch of proposals as the caller holds it.  check_proposals is everything that needs no device (and writes nothing);
// stage_proposals adds the three columns to the call's ColumnCopies — the route of every neighbouring call: ONE gather launch
// when all columns of the call lie in ibft_pinned_alloc memory, a copy command per column otherwise —;
// enqueue_proposal_digests launches proposal_digest_kernel behind them on the main stream and, if the caller wants the
// digests, their copy into the pinned mirror.  The digests stay in d_phash for whoever reads them next (block_seals_impl).
struct proposal_batch {
  const uint8_t *raw;
  const uint32_t *raw_off;
  const uint64_t *round;
  uint8_t *out_hash32;  // may be null (the _raw block calls)
  uint64_t total_blocks = 0, max_blocks = 0;  // rate blocks of all proposals / of the longest (filled by check_proposals)
};
static int check_proposals(const ibft_ctx *c, proposal_batch &p, size_t n) {
  if (n == 0) return IBFT_OK;
  if (!p.raw_off || !p.round || p.raw_off[0] != 0) return IBFT_E_INVAL;
  if (n > c->max_rows) return IBFT_E_TOOBIG;
  for (size_t i = 0; i < n; i++) {
    if (p.raw_off[i + 1] < p.raw_off[i]) return IBFT_E_INVAL;
    const uint64_t blocks = ((uint64_t)(p.raw_off[i + 1] - p.raw_off[i]) + 8u) / 136u + 1u;
    p.total_blocks += blocks;
    p.max_blocks = std::max(p.max_blocks, blocks);
  }
  if (p.raw_off[n] > c->proposal_bytes_max) return IBFT_E_TOOBIG;
  if (p.raw_off[n] && !p.raw) return IBFT_E_INVAL;
  return IBFT_OK;
}
// Which form of proposal_digest_kernel: 1 = a lane per proposal, 64 = a wavefront per proposal.  The lane form ends with its
// longest proposal (max_blocks × ≈9.4 µs) however many there are, up to a wavefront on every SIMD; the wavefront form walks a
// proposal in ≈5.3 µs per block but the chip holds only so many of them at once, so its time grows with the TOTAL number of
// blocks.  total_blocks / max_blocks is the batch's size in proposals of the longest one's length: the lane form from
// proposal_lane_rows of them on (IBFT_PROPOSAL_LANE_ROWS), and never for fewer than 64 proposals.  IBFT_PROPOSAL_LANES pins.
static uint32_t proposal_form(const ibft_ctx *c, const proposal_batch &p, size_t n) {
  if (c->proposal_lanes_force) return c->proposal_lanes_force;
  return n >= 64 && p.total_blocks >= (uint64_t)c->proposal_lane_rows * p.max_blocks ? 1u : 64u;
}
static int stage_proposals(ibft_ctx *c, ColumnCopies &cc, const proposal_batch &p, size_t n) {
  int rc;
  const size_t bytes = p.raw_off[n];
  if ((rc = ensure(c, c->d_praw, bytes + 256))) return rc;
  if ((rc = ensure(c, c->d_proff, (n + 1) * 4))) return rc;
  if ((rc = ensure(c, c->d_pround, n * 8))) return rc;
  if ((rc = ensure(c, c->d_phash, n * 32))) return rc;
  // (every call that delivers into the mirror has synchronised before it returned)
  if (p.out_hash32 && (rc = grow_pinned((void **)&c->h_phash, &c->h_phash_rows, n, 32))) return rc;
  cc.add(c->d_praw.p, p.raw, bytes);
  cc.add(c->d_proff.p, p.raw_off, (n + 1) * 4);
  cc.add(c->d_pround.p, p.round, n * 8);
  return IBFT_OK;
}
// (the launch itself, over any set of proposal buffers and on any stream: the streamed submits have a set per slot)
static int launch_proposal_digests(ibft_ctx *c, uint32_t form, const void *d_raw, const void *d_off, const void *d_round, void *d_out,
                                   size_t n, hipStream_t stream) {
  ibftk::proposal_digest_args a{};
  a.raw = (const uint8_t *)d_raw;
  a.raw_off = (const uint32_t *)d_off;
  a.round = (const uint64_t *)d_round;
  a.out32 = (uint8_t *)d_out;
  a.n = (uint32_t)n;
  if (form == 1)
    hipLaunchKernelGGL(ibftk::proposal_digest_kernel<1>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, a);
  else
    hipLaunchKernelGGL(ibftk::proposal_digest_kernel<64>, dim3((unsigned)n), dim3(64), 0, stream, a);
  HIPCHK(c, hipGetLastError());
  return IBFT_OK;
}
static int enqueue_proposal_digests(ibft_ctx *c, const proposal_batch &p, size_t n) {
  int rc;
  if ((rc = launch_proposal_digests(c, proposal_form(c, p, n), c->d_praw.p, c->d_proff.p, c->d_pround.p, c->d_phash.p, n, c->stream))) return rc;
  if (p.out_hash32) HIPCHK(c, hipMemcpyAsync(c->h_phash, c->d_phash.p, n * 32, hipMemcpyDeviceToHost, c->stream));
  return IBFT_OK;
}

int ibft_proposal_hashes(ibft_ctx *c, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round, size_t n,
                         uint8_t *out_hash32) {
  if (!c || (n && !out_hash32)) return IBFT_E_INVAL;
  proposal_batch p{raw, raw_off, round, out_hash32};
  int rc;
  if ((rc = check_proposals(c, p, n))) return rc;
  if (n == 0) return IBFT_OK;
  ctx_lock lk(c);
  HIPCHK(c, hipSetDevice(c->device));
  ColumnCopies cc;
  if ((rc = stage_proposals(c, cc, p, n))) return rc;
  if ((rc = cc.flush(c))) return rc;
  if ((rc = enqueue_proposal_digests(c, p, n))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(out_hash32, c->h_phash, n * 32);
  return IBFT_OK;
}

// ---- chain sync: the sixteen block calls --------------------------------------------------------------------------------------
// {verify, recover} × {hashes, proposals} × {one set, a set per block} × {synchronous, streamed}.  Every entry point fills a
// block_batch with what it was given and hands it to one of two implementations, which share their parts (the checks below,
// enqueue_block_head, enqueue_recover, enqueue_block_tally) and are NOT one path: the synchronous calls have another latency
// and another refusal set than a submit + collect.
constexpr bool BARE = true, SETS = true;
struct block_batch {
  const uint8_t *block_hash32;  // the blocks' hashes, or …
  proposal_batch *props;        // … the _raw calls: their proposals, hashed on the device into what then plays the uploaded hashes' part
  const uint32_t *seal_off;
  size_t n_blocks;
  const uint8_t *sig65, *signer20, *pre_flags;
  bool bare = false;  // the recover calls: no signer20 column; the emitting kernels fill the columns the caller gets and the tally reads
  bool sets = false;  // the _sets calls: block b is judged under set block_set[b] of the installed family
  const uint32_t *block_set = nullptr;
  uint32_t widest = 0;  // rows of the largest block (picks the tally's workgroup size) and of the batch: check_block_batch's
  size_t n = 0;
  uint32_t kind() const { return (bare ? IBFT_BATCH_RECOVER : 0u) | (props ? IBFT_BATCH_RAW : 0u) | (sets ? IBFT_BATCH_SETS : 0u); }
};
// The checks every block call makes, in the order it makes them.  Before c->mu is taken (outs_missing: an out buffer of a
// synchronous call that rows need is null; a submit has none) …
static int check_block_batch(const ibft_ctx *c, block_batch &b, bool outs_missing) {
  if (!c || !b.seal_off || b.seal_off[0] != 0) return IBFT_E_INVAL;
  if (b.n_blocks > c->max_rows) return IBFT_E_TOOBIG;  // (max_rows never changes after ibft_ctx_create)
  for (size_t i = 0; i < b.n_blocks; i++) {
    if (b.seal_off[i + 1] < b.seal_off[i]) return IBFT_E_INVAL;
    b.widest = std::max(b.widest, b.seal_off[i + 1] - b.seal_off[i]);
  }
  if ((b.n = b.seal_off[b.n_blocks]) > c->max_rows) return IBFT_E_TOOBIG;
  if (b.n && ((!b.props && !b.block_hash32) || !b.sig65 || (!b.bare && !b.signer20) || outs_missing)) return IBFT_E_INVAL;
  if (b.sets && b.n_blocks && !b.block_set) return IBFT_E_INVAL;
  return IBFT_OK;
}
// … and under it: each kind of batch needs only its own kind of set; a set the family does not have is refused on the host
// (no launch ever sees one); then the proposals' arguments.
static int check_block_batch_locked(const ibft_ctx *c, block_batch &b) {
  if (b.sets ? !c->fam.have : !c->have_valset) return IBFT_E_NOVALSET;
  if (b.sets)
    for (size_t i = 0; i < b.n_blocks; i++)
      if (b.block_set[i] >= c->fam.n_sets) return IBFT_E_INVAL;
  return b.props ? check_proposals(c, *b.props, b.n_blocks) : IBFT_OK;
}
// block_head_kernel on the main stream: the digests of nb blocks over the nr rows of the resident offsets, into the hash column
// the verdict kernels read.  convert: the seal-digest convention per row, the digests left as they are (a streamed batch, whose
// digests leave for the host meanwhile); otherwise a plain copy of digests the caller converted once per block.
static int enqueue_block_head(ibft_ctx *c, const void *d_digests, uint32_t nb, uint32_t nr, bool convert) {
  ibftk::block_head_args h{(const uint64_t *)d_digests, (const uint32_t *)c->d_boff.p, (uint8_t *)c->d_hash.p, nb, nr,
                            convert && c->seal_digest_mode != 0 ? 1u : 0u};
  memcpy(h.suffix_words, c->seal_suffix_words, sizeof h.suffix_words);
  hipLaunchKernelGGL(ibftk::block_head_kernel, dim3((nr + 255) / 256), dim3(256), 0, c->stream, h);
  HIPCHK(c, hipGetLastError());
  return IBFT_OK;
}

// The per-block records for nb blocks.  Nothing writes the old ones now: a synchronous call that delivered into them has
// synchronised before it returned, the streamed batch that used them last (k − 2) has been collected.
static int ensure_block_records(ibft_ctx *c, BlockRecords &r, uint32_t nb) {
  int rc;
  if (nb > r.blocks) {
    r.map = nullptr;
    if ((rc = grow_pinned((void **)&r.h, &r.blocks, nb, 32))) return rc;
    void *d = nullptr;  // the tally writes the records itself where the verdict words go there too (not under IBFT_NO_HOST_DIRECT)
    if (c->dh_mask && hipHostGetDevicePointer(&d, r.h, 0) == hipSuccess) r.map = (uint64_t *)d;
  }
  if (!r.map && (rc = ensure(c, r.d, (size_t)nb * 32))) return rc;
  return IBFT_OK;
}

// The synchronous calls: one upload, one verdict launch over every row (the AUTO rule sees the TOTAL row count), one segmented
// tally (block_tally_kernel), one synchronisation.
struct block_outputs {
  uint8_t *signer20;  // (these two: the recover calls)
  int32_t *vidx;
  uint64_t *mask;
  ibft_tally_t *tally;
};
static int block_seals_impl(ibft_ctx *c, block_batch b, const block_outputs &o) {
  int rc;
  if ((rc = check_block_batch(c, b, (b.bare && !o.signer20) || !o.mask))) return rc;
  ctx_lock lk(c);
  if ((rc = check_block_batch_locked(c, b))) return rc;
  // sets: from here to the return "the validator set" of the context is the family's union (table, size, key-cache slots)
  family_view fv(c, b.sets);
  HIPCHK(c, hipSetDevice(c->device));
  proposal_batch *const props = b.props;
  const uint32_t nb = (uint32_t)b.n_blocks, nr = (uint32_t)b.n;
  c->wire.columns = false;
  // the proposals are hashed when rows wait for the hashes or the caller wants them
  const bool hash_here = props && nb && (nr || props->out_hash32);
  ColumnCopies cc;
  if (hash_here && (rc = stage_proposals(c, cc, *props, nb))) return rc;
  if (nr) {
    if ((rc = ensure(c, c->d_boff, ((size_t)nb + 1) * 4))) return rc;
    if ((rc = ensure(c, c->d_bhash, (size_t)nb * 32))) return rc;
    if ((rc = ensure_block_records(c, c->brec, nb))) return rc;
    cc.add(c->d_boff.p, b.seal_off, ((size_t)nb + 1) * 4);
    if (b.sets) {
      if ((rc = ensure(c, c->fam.d_bset, (size_t)nb * 4))) return rc;
      cc.add(c->fam.d_bset.p, b.block_set, (size_t)nb * 4);
    }
    if (!props) cc.add(c->d_bhash.p, b.block_hash32, (size_t)nb * 32);
    cc.add(c->d_sig.p, b.sig65, b.n * 65);
    if (!b.bare) cc.add(c->d_signer.p, b.signer20, b.n * 20);
    if (b.pre_flags) cc.add(c->d_pre.p, b.pre_flags, b.n);
  }
  if ((rc = cc.flush(c))) return rc;
  // (the digests' copy out is enqueued here, in front of the seal-digest convention that converts them in place)
  if (hash_here && (rc = enqueue_proposal_digests(c, *props, nb))) return rc;
  if (nr) {  // the convention once per BLOCK — one Keccak per block instead of one per row —, then the plain spread
    void *d_block_hash = props ? c->d_phash.p : c->d_bhash.p;
    if ((rc = apply_seal_digest(c, d_block_hash, nb))) return rc;
    if ((rc = enqueue_block_head(c, d_block_hash, nb, nr, false))) return rc;
  }
  // the rows are the resident batch from here on, exactly as ibft_seals_stage would have left them (not under a family: rows
  // judged against the union are nothing ibft_seals_launch could re-judge under the single set)
  c->staged_n = b.sets ? 0 : nr;
  c->staged_pre = b.pre_flags != nullptr;
  if (nr) {
    if ((rc = enqueue_recover(c, c->stream, nr, c->staged_pre, b.bare ? ibftk::MODE_EMIT : ibftk::MODE_SEALS, next_pass_timed(c)))) return rc;
    if ((rc = enqueue_block_tally(c, nb, nr, b.widest, c->dh_mask, c->brec.map ? c->brec.map : (uint64_t *)c->brec.d.p, b.sets))) return rc;
    if (b.bare && (rc = copy_emitted(c, nr, o.signer20, o.vidx))) return rc;
    c->host_direct = false;
    const size_t mw = (size_t)mask_words(nr);
    if (!c->dh_mask) HIPCHK(c, hipMemcpyAsync(c->h_mask, c->d_mask_out.p, mw * 8, hipMemcpyDeviceToHost, c->stream));
    if (!c->brec.map) HIPCHK(c, hipMemcpyAsync(c->brec.h, c->brec.d.p, (size_t)nb * 32, hipMemcpyDeviceToHost, c->stream));
    if (c->cache_on) HIPCHK(c, hipMemcpyAsync(c->h_tally + 4, c->dev->d_learned.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->cache_on) {  // keys these rows taught the device → tables (the next call is warm)
      const uint32_t *lw = reinterpret_cast<const uint32_t *>(c->h_tally + 4);
      if ((rc = build_new_tables(c, lw[0], lw[1]))) return rc;
    }
    memcpy(o.mask, c->h_mask, mw * 8);
    if (nr & 63) o.mask[mw - 1] &= (~0ull) >> (64 - (nr & 63));
  } else if (hash_here) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (hash_here && props->out_hash32) memcpy(props->out_hash32, c->h_phash, (size_t)nb * 32);
  if (b.bare) c->staged_n = 0;  // (as after ibft_recover_seals: bare rows are no resident batch)
  fill_block_tallies(o.tally, nb, nr, c->brec.h, [&](uint32_t blk) -> const uint64_t * {
    return b.sets ? &c->fam.quorum[(size_t)b.block_set[blk] * ibftk::TALLY_SUM_WORDS] : c->quorum_w;
  });
  return IBFT_OK;
}

int ibft_verify_block_seals(ibft_ctx *c, const uint8_t *block_hash32, const uint32_t *seal_off, size_t n_blocks,
                            const uint8_t *sig65, const uint8_t *signer20, const uint8_t *pre_flags, uint64_t *out_mask,
                            ibft_tally_t *out_tally) {
  return block_seals_impl(c, {block_hash32, nullptr, seal_off, n_blocks, sig65, signer20, pre_flags}, {nullptr, nullptr, out_mask, out_tally});
}
int ibft_recover_block_seals(ibft_ctx *c, const uint8_t *block_hash32, const uint32_t *seal_off, size_t n_blocks,
                             const uint8_t *sig65, const uint8_t *pre_flags, uint8_t *out_signer20, int32_t *out_vidx,
                             uint64_t *out_mask, ibft_tally_t *out_tally) {
  return block_seals_impl(c, {block_hash32, nullptr, seal_off, n_blocks, sig65, nullptr, pre_flags, BARE}, {out_signer20, out_vidx, out_mask, out_tally});
}
int ibft_verify_block_seals_raw(ibft_ctx *c, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                const uint32_t *seal_off, size_t n_blocks, const uint8_t *sig65, const uint8_t *signer20,
                                const uint8_t *pre_flags, uint8_t *out_block_hash32, uint64_t *out_mask, ibft_tally_t *out_tally) {
  proposal_batch p{raw, raw_off, round, out_block_hash32};
  return block_seals_impl(c, {nullptr, &p, seal_off, n_blocks, sig65, signer20, pre_flags}, {nullptr, nullptr, out_mask, out_tally});
}
int ibft_recover_block_seals_raw(ibft_ctx *c, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                 const uint32_t *seal_off, size_t n_blocks, const uint8_t *sig65, const uint8_t *pre_flags,
                                 uint8_t *out_block_hash32, uint8_t *out_signer20, int32_t *out_vidx, uint64_t *out_mask,
                                 ibft_tally_t *out_tally) {
  proposal_batch p{raw, raw_off, round, out_block_hash32};
  return block_seals_impl(c, {nullptr, &p, seal_off, n_blocks, sig65, nullptr, pre_flags, BARE}, {out_signer20, out_vidx, out_mask, out_tally});
}
int ibft_verify_block_seals_sets(ibft_ctx *c, const uint8_t *block_hash32, const uint32_t *seal_off, const uint32_t *block_set,
                                 size_t n_blocks, const uint8_t *sig65, const uint8_t *signer20, const uint8_t *pre_flags,
                                 uint64_t *out_mask, ibft_tally_t *out_tally) {
  return block_seals_impl(c, {block_hash32, nullptr, seal_off, n_blocks, sig65, signer20, pre_flags, !BARE, SETS, block_set}, {nullptr, nullptr, out_mask, out_tally});
}
int ibft_recover_block_seals_sets(ibft_ctx *c, const uint8_t *block_hash32, const uint32_t *seal_off, const uint32_t *block_set,
                                  size_t n_blocks, const uint8_t *sig65, const uint8_t *pre_flags, uint8_t *out_signer20,
                                  int32_t *out_vidx, uint64_t *out_mask, ibft_tally_t *out_tally) {
  return block_seals_impl(c, {block_hash32, nullptr, seal_off, n_blocks, sig65, nullptr, pre_flags, BARE, SETS, block_set}, {out_signer20, out_vidx, out_mask, out_tally});
}
// … and from the proposals: ibft_proposal_hashes + the call above in one (the _sets call's checks in its order, then those of
// the proposals' arguments)
int ibft_verify_block_seals_sets_raw(ibft_ctx *c, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                     const uint32_t *seal_off, const uint32_t *block_set, size_t n_blocks, const uint8_t *sig65,
                                     const uint8_t *signer20, const uint8_t *pre_flags, uint8_t *out_block_hash32, uint64_t *out_mask,
                                     ibft_tally_t *out_tally) {
  proposal_batch p{raw, raw_off, round, out_block_hash32};
  return block_seals_impl(c, {nullptr, &p, seal_off, n_blocks, sig65, signer20, pre_flags, !BARE, SETS, block_set}, {nullptr, nullptr, out_mask, out_tally});
}
int ibft_recover_block_seals_sets_raw(ibft_ctx *c, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                      const uint32_t *seal_off, const uint32_t *block_set, size_t n_blocks, const uint8_t *sig65,
                                      const uint8_t *pre_flags, uint8_t *out_block_hash32, uint8_t *out_signer20, int32_t *out_vidx,
                                      uint64_t *out_mask, ibft_tally_t *out_tally) {
  proposal_batch p{raw, raw_off, round, out_block_hash32};
  return block_seals_impl(c, {nullptr, &p, seal_off, n_blocks, sig65, nullptr, pre_flags, BARE, SETS, block_set}, {out_signer20, out_vidx, out_mask, out_tally});
}

// ---- streamed chain sync: the same eight batches, enqueued and not waited for ------------------------------------------------
// Up to two batches in flight; the copy of batch k + 1 (copy stream, into the spare column set) runs under the kernels of batch
// k (main stream).  Checks: the synchronous sibling's, in its order, minus the out buffers; then the pipeline's refusals.  The
// blocks' digests (the slot's phash: uploaded hashes, or proposal_digest_kernel's) are private to the slot and only read —
// block_head_kernel applies the seal-digest convention, the one in force at the submit, while it spreads them over the rows —,
// a recover batch emits into columns of its slot, and digests / signers / indices leave on ostream (see BlockSlot).
// sets: the same path under a family of sets — the verdict kernels judge against the family's union (family_view),
// block_head_kernel is followed by the SETS form of block_tally_kernel over the slot's own block_set column, and the quorum
// words the collect hands out are copied into the slot, so the family may be replaced while the batch is in flight.

// The refusals every streamed block submit makes once its arguments are in order (c->mu held); a refused call takes no slot.
static int block_pipeline_refusal(ibft_ctx *c) {
  if (c->pass_issued != c->pass_collected || c->next_valid) {  // the two pipelines share the result slots and the spare columns
    c->last_error = c->next_valid ? "a batch staged by ibft_seals_stage_next awaits its ibft_seals_swap"
                                  : "seal passes in flight: call ibft_seals_collect first";
    return IBFT_E_INVAL;
  }
  if (c->bs_issued - c->bs_collected >= 2) {
    c->last_error = "two block batches already in flight: call ibft_block_seals_collect first";
    return IBFT_E_INVAL;
  }
  if (c->learn_rc != IBFT_OK) {  // the table build behind an already delivered batch failed (ibft_block_seals_collect): say so once
    const int rc = c->learn_rc;
    c->learn_rc = IBFT_OK;
    return rc;
  }
  return IBFT_OK;
}
// Everything a submit only RESERVES, in one place: the slot's events and ostream (whatever the batch holds), then what a batch
// with rows or proposals needs.  Nothing of the batch is enqueued here.  Everything of the slot is free: the batch that used
// it last (k − 2) has been collected — its kernels and its copies out are done (hipFree waits for the device besides: a
// buffer that grows here is read by nothing any more).
static int reserve_block_slot(ibft_ctx *c, BlockSlot &sl, const block_batch &b, bool hash_here) {
  int rc;
  const uint32_t nb = (uint32_t)b.n_blocks, nr = (uint32_t)b.n;
  for (hipEvent_t *e : {&sl.ev, &sl.ev_dig, &sl.ev_out})
    if (!*e) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
  if (!c->ostream) HIPCHK(c, hipStreamCreateWithFlags(&c->ostream, hipStreamNonBlocking));
  if (!nr && !hash_here) return IBFT_OK;
  if ((rc = ensure_result_slots(c))) return rc;
  if ((rc = ensure_spare_columns(c))) return rc;
  if ((rc = ensure(c, sl.phash, (size_t)nb * 32))) return rc;
  if (hash_here) {
    if ((rc = ensure(c, sl.praw, (size_t)b.props->raw_off[nb] + 256))) return rc;
    if ((rc = ensure(c, sl.proff, ((size_t)nb + 1) * 4))) return rc;
    if ((rc = ensure(c, sl.pround, (size_t)nb * 8))) return rc;
    if ((rc = grow_pinned((void **)&sl.h_hash, &sl.h_hash_blocks, nb, 32))) return rc;
  }
  if (nr) {
    if ((rc = ensure(c, c->d_boff_nx, ((size_t)nb + 1) * 4))) return rc;
    if ((rc = ensure_block_records(c, sl.rec, nb))) return rc;
    if (b.sets && (rc = ensure(c, sl.bset, (size_t)nb * 4))) return rc;
    if (b.bare) {
      const size_t m = std::max<size_t>(c->max_rows, c->row_cap);  // (the sizes alloc_rows gives d_signer_out / d_vidx)
      if ((rc = ensure(c, sl.signer, m * 20))) return rc;
      if ((rc = ensure(c, sl.vidx, m * 4))) return rc;
      if ((rc = grow_pinned((void **)&sl.h_signer, &sl.h_rows, nr, 20))) return rc;
      if ((rc = grow_pinned((void **)&sl.h_vidx, &sl.h_vidx_rows, nr, 4))) return rc;
    }
  }
  return IBFT_OK;
}
// d_signer_out / d_vidx ↔ the emit columns of a slot while a recover batch's kernels are enqueued (make_args and the tally
// read the context's fields); put back on every way out
struct emit_columns_view {
  ibft_ctx *c;
  BlockSlot &sl;
  bool on;
  void exchange() {
    std::swap(c->d_signer_out, sl.signer);
    std::swap(c->d_vidx, sl.vidx);
  }
  emit_columns_view(ibft_ctx *cc, BlockSlot &slot, bool on_) : c(cc), sl(slot), on(on_) {
    if (on) exchange();
  }
  ~emit_columns_view() {
    if (on) exchange();
  }
  emit_columns_view(const emit_columns_view &) = delete;
  emit_columns_view &operator=(const emit_columns_view &) = delete;
};
static int block_seals_submit_impl(ibft_ctx *c, block_batch b) {
  int rc;
  if ((rc = check_block_batch(c, b, false))) return rc;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself; side-stream tallies are joined below)
  if ((rc = check_block_batch_locked(c, b))) return rc;
  if ((rc = block_pipeline_refusal(c))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = join_side(c))) return rc;
  // sets: from here to the return "the validator set" of the context is the family's union, as in block_seals_impl.  The
  // batch is judged under the family installed NOW: its kernels read the family's device tables, which an install lets go
  // only behind them (set_validator_sets_impl), and what the collect needs of the family is copied into the slot below.
  family_view fv(c, b.sets);
  proposal_batch *const props = b.props;
  const uint32_t s = c->bs_issued & 1u, nb = (uint32_t)b.n_blocks, nr = (uint32_t)b.n;
  BlockSlot &sl = c->bs[s];
  // sets: the quorum words the collect hands out, kept in the slot (free: batch k − 2 has been collected) before anything
  // is enqueued — 16 B per block, or 4 B per block + 16 B per set of the family, whichever is smaller
  sl.setq.clear();
  sl.setidx.clear();
  if (b.sets) {
    const ValFamily &f = c->fam;
    const bool per_block = 16ull * nb <= 4ull * nb + 16ull * f.n_sets;
    const uint32_t entries = per_block ? nb : f.n_sets;
    sl.setq.reserve(2 * (size_t)entries);
    for (uint32_t e = 0; e < entries; e++) {
      const uint64_t *q = &f.quorum[(size_t)(per_block ? b.block_set[e] : e) * ibftk::TALLY_SUM_WORDS];
      sl.setq.push_back(q[0]);
      sl.setq.push_back(q[1]);
    }
    if (!per_block) sl.setidx.assign(b.block_set, b.block_set + nb);
  }
  // submitted raw: the proposals are hashed whether or not rows wait for the hashes — the collect may ask for them
  const bool hash_here = props && nb;
  bool has_out = false;
  if ((rc = reserve_block_slot(c, sl, b, hash_here))) return rc;
  if (nr || hash_here) {
    const size_t raw_bytes = hash_here ? props->raw_off[nb] : 0;
    // ---- the copy stream: proposals (and, where told to, their digests), then the seal columns into the spare set
    if (hash_here) {
      if (raw_bytes) HIPCHK(c, hipMemcpyAsync(sl.praw.p, props->raw, raw_bytes, hipMemcpyHostToDevice, c->cstream));
      HIPCHK(c, hipMemcpyAsync(sl.proff.p, props->raw_off, ((size_t)nb + 1) * 4, hipMemcpyHostToDevice, c->cstream));
      HIPCHK(c, hipMemcpyAsync(sl.pround.p, props->round, (size_t)nb * 8, hipMemcpyHostToDevice, c->cstream));
    } else if (!props) {
      HIPCHK(c, hipMemcpyAsync(sl.phash.p, b.block_hash32, (size_t)nb * 32, hipMemcpyHostToDevice, c->cstream));
    }
    const uint32_t form = hash_here ? proposal_form(c, *props, nb) : 0u;  // (the form is chosen here: pinned at the submit)
    if (hash_here && c->stream_digest_copy) {
      // behind the copy of its bytes, next to whatever the main stream runs: batch k's verdict kernel in a loop that keeps one in flight
      if ((rc = launch_proposal_digests(c, form, sl.praw.p, sl.proff.p, sl.pround.p, sl.phash.p, nb, c->cstream))) return rc;
      HIPCHK(c, hipEventRecord(sl.ev_dig, c->cstream));
    }
    if (nr) {
      // The spare set was the resident one until the previous swap: kernels enqueued before it — a tally reads the offsets —
      // may still be at it.  ev_cols_read was recorded behind them.
      HIPCHK(c, hipStreamWaitEvent(c->cstream, c->ev_cols_read, 0));
      HIPCHK(c, hipMemcpyAsync(c->d_boff_nx.p, b.seal_off, ((size_t)nb + 1) * 4, hipMemcpyHostToDevice, c->cstream));
      if (b.sets) HIPCHK(c, hipMemcpyAsync(sl.bset.p, b.block_set, (size_t)nb * 4, hipMemcpyHostToDevice, c->cstream));
      HIPCHK(c, hipMemcpyAsync(c->d_sig_nx.p, b.sig65, b.n * 65, hipMemcpyHostToDevice, c->cstream));
      if (!b.bare) HIPCHK(c, hipMemcpyAsync(c->d_signer_nx.p, b.signer20, b.n * 20, hipMemcpyHostToDevice, c->cstream));
      if (b.pre_flags) HIPCHK(c, hipMemcpyAsync(c->d_pre_nx.p, b.pre_flags, b.n, hipMemcpyHostToDevice, c->cstream));
    }
    HIPCHK(c, hipEventRecord(c->ev_staged, c->cstream));
    if (nr) HIPCHK(c, hipEventRecord(c->ev_cols_read, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_staged, 0));
    // from here on a failure leaves commands of this batch on the streams: nothing of it is delivered, the slot stays free
    if (hash_here && !c->stream_digest_copy) {
      if ((rc = launch_proposal_digests(c, form, sl.praw.p, sl.proff.p, sl.pround.p, sl.phash.p, nb, c->stream))) return rc;
      HIPCHK(c, hipEventRecord(sl.ev_dig, c->stream));
    }
    if (hash_here) {  // the digests go out as computed, next to everything that follows on the main stream
      HIPCHK(c, hipStreamWaitEvent(c->ostream, sl.ev_dig, 0));
      HIPCHK(c, hipMemcpyAsync(sl.h_hash, sl.phash.p, (size_t)nb * 32, hipMemcpyDeviceToHost, c->ostream));
      has_out = true;
    }
    if (nr) {
      std::swap(c->d_sig, c->d_sig_nx);
      std::swap(c->d_signer, c->d_signer_nx);
      std::swap(c->d_pre, c->d_pre_nx);
      std::swap(c->d_boff, c->d_boff_nx);
      c->wire.columns = false;
      // verify kind: the rows are the resident batch from here on; bare rows are none, and neither are rows judged against a
      // family's union (as after the synchronous siblings)
      c->staged_n = b.bare || b.sets ? 0 : nr;
      c->staged_pre = b.pre_flags != nullptr;
      if ((rc = enqueue_block_head(c, sl.phash.p, nb, nr, true))) return rc;
      const bool time_it = next_pass_timed(c);
      const bool direct = sl.rec.map != nullptr;
      {
        emit_columns_view ev(c, sl, b.bare);
        if ((rc = enqueue_recover(c, c->stream, nr, b.pre_flags != nullptr, b.bare ? ibftk::MODE_EMIT : ibftk::MODE_SEALS, time_it))) return rc;
        if ((rc = enqueue_block_tally(c, nb, nr, b.widest, direct ? c->dp_mask[s] : nullptr,
                                      direct ? sl.rec.map : (uint64_t *)sl.rec.d.p, b.sets, sl.bset.p)))
          return rc;
      }
      c->host_direct = false;
      if (!direct) {
        HIPCHK(c, hipMemcpyAsync(c->p_mask[s], c->d_mask_out.p, (size_t)mask_words(nr) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(sl.rec.h, sl.rec.d.p, (size_t)nb * 32, hipMemcpyDeviceToHost, c->stream));
      }
      if (c->cache_on) HIPCHK(c, hipMemcpyAsync(c->p_tally[s] + 4, c->dev->d_learned.p, 8, hipMemcpyDeviceToHost, c->stream));
    }
  }
  HIPCHK(c, hipEventRecord(sl.ev, c->stream));
  if (b.bare && nr) {  // signers and indices: behind the tally, off the main stream — the next batch's kernels do not wait for 24 B per row
    HIPCHK(c, hipStreamWaitEvent(c->ostream, sl.ev, 0));
    HIPCHK(c, hipMemcpyAsync(sl.h_signer, sl.signer.p, b.n * 20, hipMemcpyDeviceToHost, c->ostream));
    HIPCHK(c, hipMemcpyAsync(sl.h_vidx, sl.vidx.p, b.n * 4, hipMemcpyDeviceToHost, c->ostream));
    has_out = true;
  }
  if (has_out) HIPCHK(c, hipEventRecord(sl.ev_out, c->ostream));
  sl.rows = nr;
  sl.blocks = nb;
  memcpy(sl.quorum, c->quorum_w, sizeof sl.quorum);
  sl.kind = b.kind();
  sl.has_out = has_out;
  c->bs_issued++;
  return IBFT_OK;
}
int ibft_block_seals_submit(ibft_ctx *c, const uint8_t *block_hash32, const uint32_t *seal_off, size_t n_blocks,
                            const uint8_t *sig65, const uint8_t *signer20, const uint8_t *pre_flags) {
  return block_seals_submit_impl(c, {block_hash32, nullptr, seal_off, n_blocks, sig65, signer20, pre_flags});
}
int ibft_block_seals_submit_raw(ibft_ctx *c, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round, const uint32_t *seal_off,
                                size_t n_blocks, const uint8_t *sig65, const uint8_t *signer20, const uint8_t *pre_flags) {
  proposal_batch p{raw, raw_off, round, nullptr};
  return block_seals_submit_impl(c, {nullptr, &p, seal_off, n_blocks, sig65, signer20, pre_flags});
}
int ibft_recover_block_seals_submit(ibft_ctx *c, const uint8_t *block_hash32, const uint32_t *seal_off, size_t n_blocks,
                                    const uint8_t *sig65, const uint8_t *pre_flags) {
  return block_seals_submit_impl(c, {block_hash32, nullptr, seal_off, n_blocks, sig65, nullptr, pre_flags, BARE});
}
int ibft_recover_block_seals_submit_raw(ibft_ctx *c, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                        const uint32_t *seal_off, size_t n_blocks, const uint8_t *sig65, const uint8_t *pre_flags) {
  proposal_batch p{raw, raw_off, round, nullptr};
  return block_seals_submit_impl(c, {nullptr, &p, seal_off, n_blocks, sig65, nullptr, pre_flags, BARE});
}
// The same four under a family of sets (IBFT_BATCH_SETS): the streamed forms of the _sets / _sets_raw calls.
int ibft_block_seals_submit_sets(ibft_ctx *c, const uint8_t *block_hash32, const uint32_t *seal_off, const uint32_t *block_set,
                                 size_t n_blocks, const uint8_t *sig65, const uint8_t *signer20, const uint8_t *pre_flags) {
  return block_seals_submit_impl(c, {block_hash32, nullptr, seal_off, n_blocks, sig65, signer20, pre_flags, !BARE, SETS, block_set});
}
int ibft_block_seals_submit_sets_raw(ibft_ctx *c, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                     const uint32_t *seal_off, const uint32_t *block_set, size_t n_blocks, const uint8_t *sig65,
                                     const uint8_t *signer20, const uint8_t *pre_flags) {
  proposal_batch p{raw, raw_off, round, nullptr};
  return block_seals_submit_impl(c, {nullptr, &p, seal_off, n_blocks, sig65, signer20, pre_flags, !BARE, SETS, block_set});
}
int ibft_recover_block_seals_submit_sets(ibft_ctx *c, const uint8_t *block_hash32, const uint32_t *seal_off, const uint32_t *block_set,
                                         size_t n_blocks, const uint8_t *sig65, const uint8_t *pre_flags) {
  return block_seals_submit_impl(c, {block_hash32, nullptr, seal_off, n_blocks, sig65, nullptr, pre_flags, BARE, SETS, block_set});
}
int ibft_recover_block_seals_submit_sets_raw(ibft_ctx *c, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                             const uint32_t *seal_off, const uint32_t *block_set, size_t n_blocks, const uint8_t *sig65,
                                             const uint8_t *pre_flags) {
  proposal_batch p{raw, raw_off, round, nullptr};
  return block_seals_submit_impl(c, {nullptr, &p, seal_off, n_blocks, sig65, nullptr, pre_flags, BARE, SETS, block_set});
}

// The oldest batch in flight → the caller.  ex: ibft_block_seals_collect_ex (digests, signers and indices where the batch's
// kind carries them); the old call delivers verdict words and records only and refuses a recover batch with rows.
static int block_seals_collect_impl(ibft_ctx *c, bool ex, uint8_t *out_block_hash32, uint8_t *out_signer20, int32_t *out_vidx,
                                    uint64_t *out_mask, ibft_tally_t *out_tally) {
  if (!c) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself)
  if (c->bs_collected == c->bs_issued) {
    c->last_error = ex ? "ibft_block_seals_collect_ex without a submitted batch" : "ibft_block_seals_collect without a submitted batch";
    return IBFT_E_INVAL;
  }
  const uint32_t s = c->bs_collected & 1u;
  BlockSlot &sl = c->bs[s];
  const uint32_t nr = sl.rows, nb = sl.blocks, kind = sl.kind;
  if (nr && !out_mask) return IBFT_E_INVAL;
  if ((kind & IBFT_BATCH_RECOVER) && nr) {  // refused before anything is written: the batch stays in flight
    if (!ex) {
      c->last_error = "the oldest batch recovers signers: collect it with ibft_block_seals_collect_ex";
      return IBFT_E_INVAL;
    }
    if (!out_signer20) {
      c->last_error = "ibft_block_seals_collect_ex: a recover batch with rows needs out_signer20";
      return IBFT_E_INVAL;
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(sl.ev));
  if (sl.has_out) HIPCHK(c, hipEventSynchronize(sl.ev_out));
  if (nr) {
    const size_t mw = (size_t)mask_words(nr);
    memcpy(out_mask, c->p_mask[s], mw * 8);
    if (nr & 63) out_mask[mw - 1] &= (~0ull) >> (64 - (nr & 63));
  }
  // (a sets batch: the quorum words kept at its submit — c->fam may be another family by now)
  fill_block_tallies(out_tally, nb, nr, sl.rec.h, [&](uint32_t b) -> const uint64_t * {
    if (!(kind & IBFT_BATCH_SETS)) return sl.quorum;
    return &sl.setq[2 * (size_t)(sl.setidx.empty() ? b : sl.setidx[b])];
  });
  if (ex && (kind & IBFT_BATCH_RAW) && out_block_hash32 && nb) memcpy(out_block_hash32, sl.h_hash, (size_t)nb * 32);
  if (ex && (kind & IBFT_BATCH_RECOVER) && nr) {
    memcpy(out_signer20, sl.h_signer, (size_t)nr * 20);
    if (out_vidx) memcpy(out_vidx, sl.h_vidx, (size_t)nr * 4);
  }
  // The batch is DELIVERED before anything else can fail (the rule of ibft_seals_collect).
  c->bs_collected++;
  // a sets batch taught keys of a family's union.  This — behind the delivery — is the one place where a collect reads
  // c->fam: the build counts against the union installed NOW (the pool's build pass itself serves every slot of the device,
  // whoever holds it), which may be another family than the batch's
  family_view fv(c, (kind & IBFT_BATCH_SETS) != 0);
  if (c->cache_on && nr) {  // keys this batch taught the device → tables (build_new_tables drains the main stream when there
                            // are any — a newer batch in flight included; its results wait in their slot)
    const uint32_t *lw = reinterpret_cast<const uint32_t *>(c->p_tally[s] + 4);
    const int rcb = build_new_tables(c, lw[0], lw[1]);
    if (rcb) c->learn_rc = rcb;
  }
  return IBFT_OK;
}
int ibft_block_seals_collect(ibft_ctx *c, uint64_t *out_mask, ibft_tally_t *out_tally) {
  return block_seals_collect_impl(c, false, nullptr, nullptr, nullptr, out_mask, out_tally);
}
int ibft_block_seals_collect_ex(ibft_ctx *c, uint8_t *out_block_hash32, uint8_t *out_signer20, int32_t *out_vidx, uint64_t *out_mask,
                                ibft_tally_t *out_tally) {
  return block_seals_collect_impl(c, true, out_block_hash32, out_signer20, out_vidx, out_mask, out_tally);
}

// Batches in flight, rows, blocks and kind of the oldest (0 when none): a binding sizes its buffers from these.
int ibft_block_seals_pending_ex(ibft_ctx *c, uint32_t *batches_in_flight, uint32_t *oldest_rows, uint32_t *oldest_blocks,
                                uint32_t *oldest_kind) {
  if (!c) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(c->mu);  // (a call of the pipeline itself)
  const bool any = c->bs_collected != c->bs_issued;
  const BlockSlot &oldest = c->bs[c->bs_collected & 1u];
  if (batches_in_flight) *batches_in_flight = c->bs_issued - c->bs_collected;
  if (oldest_rows) *oldest_rows = any ? oldest.rows : 0u;
  if (oldest_blocks) *oldest_blocks = any ? oldest.blocks : 0u;
  if (oldest_kind) *oldest_kind = any ? oldest.kind : 0u;
  return IBFT_OK;
}
int ibft_block_seals_pending(ibft_ctx *c, uint32_t *batches_in_flight, uint32_t *oldest_rows, uint32_t *oldest_blocks) {
  return ibft_block_seals_pending_ex(c, batches_in_flight, oldest_rows, oldest_blocks, nullptr);
}

// a3 up to and including the tally (c->mu held)
static int senders_launch_locked(ibft_ctx *c, const uint8_t *payload, const uint32_t *off, const uint8_t *sig65,
                                 const uint8_t *from20, const uint8_t *pre_flags, size_t n) {
  if (n && (!off || !sig65 || !from20)) return IBFT_E_INVAL;
  if (!offsets_ok(off, n) || !bytes_ok(off, n, payload)) return IBFT_E_INVAL;
  if (n > c->max_rows) return IBFT_E_TOOBIG;
  if (!c->have_valset) return IBFT_E_NOVALSET;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  c->wire.columns = false;
  size_t pbytes = n ? off[n] : 0;
  if ((rc = ensure(c, c->d_payload, pbytes + 256))) return rc;
  ColumnCopies cc;
  cc.add(c->d_payload.p, payload, pbytes);
  if (n) cc.add(c->d_off.p, off, (n + 1) * 4);
  cc.add(c->d_sig.p, sig65, n * 65);
  cc.add(c->d_signer.p, from20, n * 20);
  if (pre_flags) cc.add(c->d_pre.p, pre_flags, n);
  if ((rc = cc.flush(c))) return rc;
  c->staged_n = (uint32_t)n;
  c->staged_pre = pre_flags != nullptr;
  c->ev_used = 0;
  if ((rc = enqueue_recover(c, c->stream, (uint32_t)n, pre_flags != nullptr, ibftk::MODE_SENDERS, true))) return rc;
  return enqueue_tally(c, (uint32_t)n);
}

int ibft_verify_senders(ibft_ctx *c, const uint8_t *payload, const uint32_t *off, const uint8_t *sig65,
                        const uint8_t *from20, const uint8_t *pre_flags, size_t n, uint64_t *out_mask,
                        ibft_tally_t *tally) {
  if (!c || (n && (!off || !out_mask))) return IBFT_E_INVAL;
  ctx_lock lk(c);
  int rc = senders_launch_locked(c, payload, off, sig65, from20, pre_flags, n);
  if (rc) return rc;
  return fetch_results(c, (uint32_t)n, out_mask, tally, true);
}

// IBFT_FLAG_WIRE_RECODE: after wire_parse_kernel, before anything reads its columns (c->mu held, n > 0)
static int enqueue_wire_recode(ibft_ctx *c, uint32_t n) {
  if (!c->wire_recode) return IBFT_OK;
  hipLaunchKernelGGL(ibftk::wire_recode_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, (const uint8_t *)c->d_payload.p,
                     (const uint32_t *)c->d_off.p, n, (wire::row_info *)c->d_wire_rows.p, (uint8_t *)c->d_hash.p,
                     (uint8_t *)c->d_sig.p, (uint8_t *)c->d_signer.p, (uint8_t *)c->d_seal.p, (uint8_t *)c->d_pre.p);
  HIPCHK(c, hipGetLastError());
  return IBFT_OK;
}

// what both flat wire calls need in HBM: the bytes (with 256 of slack), the parse results, the seals the walk finds
static int ensure_wire_buffers(ibft_ctx *c, size_t wbytes) {
  int rc;
  if ((rc = ensure(c, c->d_payload, wbytes + 256))) return rc;
  if ((rc = ensure(c, c->d_wire_rows, (size_t)c->max_rows * sizeof(wire::row_info)))) return rc;
  return ensure(c, c->d_seal, (size_t)c->max_rows * 65 + 64);
}

// the canonical walk over the n > 0 messages in d_payload / d_off, then the recode walk where the flag asks for it
static int enqueue_wire_parse(ibft_ctx *c, uint32_t n) {
  hipLaunchKernelGGL(ibftk::wire_parse_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, (const uint8_t *)c->d_payload.p,
                     (const uint32_t *)c->d_off.p, n, (wire::row_info *)c->d_wire_rows.p, (uint8_t *)c->d_hash.p,
                     (uint8_t *)c->d_sig.p, (uint8_t *)c->d_signer.p, (uint8_t *)c->d_seal.p, (uint8_t *)c->d_pre.p);
  HIPCHK(c, hipGetLastError());
  return enqueue_wire_recode(c, n);
}

int ibft_wire_stats(ibft_ctx *c, uint32_t *rows, uint32_t *recoded_rows, uint32_t *needs_host_rows) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  uint32_t n = 0, recoded = 0, needs = 0;
  if (c->wire.parsed && c->wire.rows) {
    n = c->wire.rows;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<wire::row_info> h(n);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h.data(), c->d_wire_rows.p, (size_t)n * sizeof(wire::row_info), hipMemcpyDeviceToHost));
    for (const wire::row_info &ri : h) {
      recoded += ri.status == wire::STATUS_OK && ri.pad[0] == 1;
      needs += ri.status == wire::STATUS_NEEDS_HOST;
    }
  }
  if (rows) *rows = n;
  if (recoded_rows) *recoded_rows = recoded;
  if (needs_host_rows) *needs_host_rows = needs;
  return IBFT_OK;
}

int ibft_verify_senders_wire(ibft_ctx *c, const uint8_t *wire_bytes, const uint32_t *off, size_t n, uint64_t *out_mask,
                             ibft_wire_row_t *out_rows, ibft_tally_t *tally) {
  static_assert(sizeof(ibft_wire_row_t) == sizeof(wire::row_info), "ABI");
  if (!c || (n && (!off || !out_mask))) return IBFT_E_INVAL;
  if (!offsets_ok(off, n) || !bytes_ok(off, n, wire_bytes)) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (n > c->max_rows) return IBFT_E_TOOBIG;
  if (!c->have_valset) return IBFT_E_NOVALSET;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  const size_t wbytes = n ? off[n] : 0;
  if ((rc = ensure_wire_buffers(c, wbytes))) return rc;
  if (wbytes) HIPCHK(c, hipMemcpyAsync(c->d_payload.p, wire_bytes, wbytes, hipMemcpyHostToDevice, c->stream));
  if ((rc = upload(c, c->d_off, off, (n + 1) * 4))) return rc;
  c->staged_n = (uint32_t)n;
  c->staged_pre = true;
  c->wire.rows = (uint32_t)n;
  c->wire.columns = true;
  c->wire.begin();
  c->ev_used = 0;
  if (n && (rc = enqueue_wire_parse(c, (uint32_t)n))) return rc;
  // the digest column now holds keccak256(PayloadNoSig): the sender check is the seal-style pass (mode 0)
  if ((rc = enqueue_recover(c, c->stream, (uint32_t)n, true, ibftk::MODE_SEALS, true))) return rc;
  if ((rc = enqueue_tally(c, (uint32_t)n))) return rc;
  if (out_rows && n)
    HIPCHK(c, hipMemcpyAsync(out_rows, c->d_wire_rows.p, n * sizeof(ibft_wire_row_t), hipMemcpyDeviceToHost, c->stream));
  if ((rc = fetch_results(c, (uint32_t)n, out_mask, tally, true))) return rc;
  c->wire.parsed = true;
  return IBFT_OK;
}

// The same under a family of sets: every message judged under the set of ITS height (ibft_set_height_sets).  The walks, then
// wire_row_set_kernel (the rows' sets; rows without one pre-flagged), the verdict launch against the family's union
// (family_view), wire_sets_tally_kernel (the union verdicts → per-set verdicts, indices and records), one synchronisation.
static int enqueue_wire_sets_tally(ibft_ctx *c, uint32_t n, uint64_t *out) {
  int rc;
  if ((rc = wait_for_readers(c, c->stream))) return rc;
  const ValFamily &f = c->fam;
  const HeightSets &h = c->hsets;
  ibftk::wire_sets_tally_args t{};
  t.work_mask = (uint64_t *)c->d_mask.p;
  t.mask = (uint64_t *)c->d_mask_out.p;
  t.host_mask = c->dh_mask;
  t.vidx = (int32_t *)c->d_vidx.p;
  t.row_set = (const int32_t *)h.d_row_set.p;
  t.setidx = (const int32_t *)f.d_setidx.p;
  t.set_meta = (const uint2 *)f.d_meta.p;
  t.vpower32 = (const uint32_t *)f.d_power.p;
  t.quorum = (const uint64_t *)f.d_quorum.p;
  t.n = n;
  t.n_sets = f.n_sets;
  t.n_union = c->n_validators;  // (under family_view: the union's size)
  t.seen_words = (f.entries + 31) / 32;
  size_t dyn;
  t.lds_bitmap = bitmap_in_lds(f.entries, &dyn);
  t.seen = (uint32_t *)h.d_seen.p;
  t.set_acc = (uint64_t *)h.d_acc.p;
  t.acc = (uint64_t *)c->d_acc.p;
  t.out = out;
  const dim3 grid((n + ibftk::WSETS_ROWS - 1) / ibftk::WSETS_ROWS), block(ibftk::WSETS_THREADS);
  with_power_words(f.power_words, [&](auto PW) { hipLaunchKernelGGL(ibftk::wire_sets_tally_kernel<decltype(PW)::value>, grid, block, dyn, c->stream, t); });
  HIPCHK(c, hipGetLastError());
  mask_consumed(c, mask_words(n));
  return IBFT_OK;
}

// What ibft_verify_senders_wire_views asks for on top of the sets call (null: the sets call itself).
struct wire_views_out {
  size_t views_cap;
  int32_t *out_view;
  uint64_t *out_stored;
  ibft_wire_view_t *out_views;
  uint32_t *out_n_views;
  bool seals;          // ibft_verify_messages_wire_views: the committed seals in the same verdict launch, COMMIT records over stored ∧ sealed
  uint64_t *out_seal;  // (seals) may be null
};

// Buffers of the views stage for n rows (before anything is enqueued: ensure() may free and allocate).
static int ensure_wire_views(ibft_ctx *c, uint32_t n, uint32_t cap, uint32_t slots, bool seals) {
  WireViews &w = c->wviews;
  const size_t acc_bytes = (size_t)cap * (2 * c->fam.power_words + (seals ? 2 : 1)) * 8;
  int rc;
  if (acc_bytes > w.d_acc.cap) w.acc_dirty = true;  // a fresh allocation holds anything
  if ((rc = ensure(c, w.d_tables, (size_t)slots * 8 + 8)) || (rc = ensure(c, w.d_slots, (size_t)n * 8)) || (rc = ensure(c, w.d_rank, (size_t)n * 4)) ||
      (rc = ensure(c, w.d_first, (size_t)cap * 4)) || (rc = ensure(c, w.d_view, (size_t)n * 4)) ||
      (rc = ensure(c, w.d_stored, (size_t)mask_words(n) * 8)) || (rc = ensure(c, w.d_acc, acc_bytes)) ||
      (rc = ensure(c, w.d_recs, (size_t)cap * sizeof(ibft_wire_view_t))))
    return rc;
  if (seals && ((rc = ensure(c, w.d_sflags, n)) || (rc = ensure(c, w.d_seal_row, (size_t)n * 4)) || (rc = ensure(c, w.d_seal_src, (size_t)n * 4)) ||
                (rc = ensure(c, w.d_seal_words, 16)) || (rc = ensure(c, w.d_seal_mask, (size_t)mask_words(n) * 8))))
    return rc;
  return IBFT_OK;
}

// the family's lookup and power columns as the views and seal kernels read them (under family_view)
static wviews::family wire_views_family(const ibft_ctx *c) {
  const ValFamily &f = c->fam;
  wviews::family o{};
  o.setidx = (const int32_t *)f.d_setidx.p;
  o.set_meta = (const uint2 *)f.d_meta.p;
  o.vpower32 = (const uint32_t *)f.d_power.p;
  o.quorum = (const uint64_t *)f.d_quorum.p;
  o.vtab = (const uint32_t *)c->d_vtab.p;  // (under family_view: the union's table, mask and size)
  o.vslot_mask = c->vslot_mask;
  o.n_union = c->n_validators;
  o.n_pieces = 2 * (int)f.power_words;
  return o;
}

static ibftk::wire_seals_args wire_seals_args_of(ibft_ctx *c, uint32_t n, uint32_t half) {
  WireViews &w = c->wviews;
  ibftk::wire_seals_args a{};
  a.rows = (const wire::row_info *)c->d_wire_rows.p;
  a.row_set = (const int32_t *)c->hsets.d_row_set.p;
  a.seal65 = (const uint8_t *)c->d_seal.p;
  a.n = n;
  a.half = half;
  a.fam = wire_views_family(c);
  a.flags = (uint8_t *)w.d_sflags.p;
  a.seal_row = (uint32_t *)w.d_seal_row.p;
  a.src = (uint32_t *)w.d_seal_src.p;
  a.words = (uint32_t *)w.d_seal_words.p;
  a.hash32 = (uint8_t *)c->d_hash.p;
  a.sig65 = (uint8_t *)c->d_sig.p;
  a.signer20 = (uint8_t *)c->d_signer.p;
  a.pre_flags = (uint8_t *)c->d_pre.p;
  a.mask = (const uint64_t *)c->d_mask_out.p;
  a.work_mask = (uint64_t *)c->d_mask.p;
  a.seal_mask = (uint64_t *)w.d_seal_mask.p;
  return a;
}

// The seal rows of ibft_verify_messages_wire_views behind wire_row_set_kernel, in front of the verdict launch over half + n
// rows: mark, scan, stage (kernels.hip.h), the rows between n and half pre-flagged, the seal-digest convention over the
// dense hashes.
static int enqueue_wire_seals_stage(ibft_ctx *c, uint32_t n, uint32_t half) {
  const ibftk::wire_seals_args a = wire_seals_args_of(c, n, half);
  const dim3 grid((n + ibftk::WSEALS_THREADS - 1) / ibftk::WSEALS_THREADS), block(ibftk::WSEALS_THREADS);
  hipLaunchKernelGGL(ibftk::wire_seals_mark_kernel, grid, block, 0, c->stream, a);
  hipLaunchKernelGGL(ibftk::wire_seals_scan_kernel, dim3(1), dim3(1024), 0, c->stream, a);
  hipLaunchKernelGGL(ibftk::wire_seals_stage_kernel, grid, block, 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  if (half != n) {
    HIPCHK(c, hipMemsetAsync(a.sig65 + 65ull * n, 0, 65ull * (half - n), c->stream));
    HIPCHK(c, hipMemsetAsync(a.pre_flags + n, 1, half - n, c->stream));
  }
  return apply_seal_digest(c, a.hash32 + 32ull * half, n);
}

// … and behind wire_sets_tally_kernel: the seal half's verdict words → the rows' seal bits; the work mask is zero again.
static int enqueue_wire_seals_combine(ibft_ctx *c, uint32_t n, uint32_t half) {
  const ibftk::wire_seals_args a = wire_seals_args_of(c, n, half);
  hipLaunchKernelGGL(ibftk::wire_seals_combine_kernel, dim3((n + ibftk::WSEALS_THREADS - 1) / ibftk::WSEALS_THREADS), dim3(ibftk::WSEALS_THREADS), 0,
                     c->stream, a);
  HIPCHK(c, hipGetLastError());
  mask_consumed(c, mask_words((size_t)half + n));  // the tally zeroed the sender words, this kernel the seal words
  return IBFT_OK;
}

// The views stage behind wire_sets_tally_kernel (same stream): one fill (tables to EMPTY), then insert, rank, tally, records.  Reads the final mask (d_mask_out), the rewritten index column, the rows' sets and the parsed rows.
static int enqueue_wire_views(ibft_ctx *c, uint32_t n, uint32_t cap, uint32_t slots, bool seals) {
  WireViews &w = c->wviews;
  const ValFamily &f = c->fam;
  const CertState &s = c->cert;
  if (w.acc_dirty) HIPCHK(c, hipMemsetAsync(w.d_acc.p, 0, w.d_acc.cap, c->stream));
  w.acc_dirty = true;  // until this call has come back clean
  HIPCHK(c, hipMemsetAsync(w.d_tables.p, 0xFF, (size_t)slots * 8 + 8, c->stream));  // (the tables and the two words behind them)
  ibftk::wire_views_args a{};
  a.rows = (const wire::row_info *)c->d_wire_rows.p;
  a.vidx = (const int32_t *)c->d_vidx.p;
  a.row_set = (const int32_t *)c->hsets.d_row_set.p;
  a.mask = (const uint64_t *)c->d_mask_out.p;
  a.seal_mask = seals ? (const uint64_t *)w.d_seal_mask.p : nullptr;
  a.n = n;
  a.views_cap = cap;
  a.slots = slots;
  a.salt = w.salt;
  a.key_table = (uint32_t *)w.d_tables.p;
  a.last_table = a.key_table + slots;
  a.slot_key = (uint32_t *)w.d_slots.p;
  a.slot_last = a.slot_key + n;
  a.rank_of = (uint32_t *)w.d_rank.p;
  a.first_row = (uint32_t *)w.d_first.p;
  a.words = a.key_table + 2 * (size_t)slots;
  a.out_view = (int32_t *)w.d_view.p;
  a.out_stored = (uint64_t *)w.d_stored.p;
  a.view_acc = (uint64_t *)w.d_acc.p;
  a.out_views = (wviews::view_t *)w.d_recs.p;
  a.fam = wire_views_family(c);
  a.table = certd::proposer_table{s.prop_height, s.prop_first, (const uint8_t *)s.proposers.p, s.proposers.p ? s.prop_rounds : 0u};
  const dim3 rows_grid((n + ibftk::WVIEWS_THREADS - 1) / ibftk::WVIEWS_THREADS), block(ibftk::WVIEWS_THREADS);
  hipLaunchKernelGGL(ibftk::wire_views_insert_kernel, rows_grid, block, 0, c->stream, a);
  hipLaunchKernelGGL(ibftk::wire_views_rank_kernel, dim3(1), dim3(1024), 0, c->stream, a);
  const dim3 views_grid((cap + ibftk::WVIEWS_THREADS - 1) / ibftk::WVIEWS_THREADS);
  with_power_words(f.power_words, [&](auto PW) {
    if (!seals) {
      hipLaunchKernelGGL((ibftk::wire_views_tally_kernel<decltype(PW)::value, false>), rows_grid, block, 0, c->stream, a);
      hipLaunchKernelGGL(ibftk::wire_views_records_kernel<false>, views_grid, block, 0, c->stream, a);
    } else {
      hipLaunchKernelGGL((ibftk::wire_views_tally_kernel<decltype(PW)::value, true>), rows_grid, block, 0, c->stream, a);
      hipLaunchKernelGGL(ibftk::wire_views_records_kernel<true>, views_grid, block, 0, c->stream, a);
    }
  });
  HIPCHK(c, hipGetLastError());
  return IBFT_OK;
}

static int wire_sets_impl(ibft_ctx *c, const uint8_t *wire_bytes, const uint32_t *off, size_t n, uint64_t *out_mask, ibft_wire_row_t *out_rows,
                          int32_t *out_set, int32_t *out_vidx, ibft_tally_t *out_tally, const wire_views_out *vo);

int ibft_verify_senders_wire_sets(ibft_ctx *c, const uint8_t *wire_bytes, const uint32_t *off, size_t n, uint64_t *out_mask,
                                  ibft_wire_row_t *out_rows, int32_t *out_set, int32_t *out_vidx, ibft_tally_t *out_tally) {
  return wire_sets_impl(c, wire_bytes, off, n, out_mask, out_rows, out_set, out_vidx, out_tally, nullptr);
}

// The sets call plus one quorum record per (height, round, type, proposal hash): the sets call's checks in its order, with
// views_cap == 0 for a batch that has rows among the argument checks in front.
int ibft_verify_senders_wire_views(ibft_ctx *c, const uint8_t *wire_bytes, const uint32_t *off, size_t n, size_t views_cap, uint64_t *out_mask,
                                   ibft_wire_row_t *out_rows, int32_t *out_set, int32_t *out_vidx, ibft_tally_t *out_tally, int32_t *out_view,
                                   uint64_t *out_stored, ibft_wire_view_t *out_views, uint32_t *out_n_views) {
  static_assert(sizeof(ibft_wire_view_t) == sizeof(wviews::view_t) && sizeof(ibft_wire_view_t) == 128 && sizeof(ibft_wire_view_t) % 8 == 0, "ABI");
  static_assert(sizeof(ibft_tally_t) == sizeof(wviews::tally_t) && offsetof(ibft_wire_view_t, tally) == offsetof(wviews::view_t, tally) &&
                    offsetof(ibft_wire_view_t, proposal_hash) == offsetof(wviews::view_t, proposal_hash),
                "ABI");
  const wire_views_out vo{views_cap, out_view, out_stored, out_views, out_n_views, false, nullptr};
  return wire_sets_impl(c, wire_bytes, off, n, out_mask, out_rows, out_set, out_vidx, out_tally, &vo);
}

// The views call with the committed seals of the COMMIT rows judged in the SAME verdict launch (sender rows [0, n), the
// sealable rows' seals dense from ⌈n/64⌉·64 on) and the COMMIT records tallied over stored ∧ sealed: the views call's checks
// in its order.
int ibft_verify_messages_wire_views(ibft_ctx *c, const uint8_t *wire_bytes, const uint32_t *off, size_t n, size_t views_cap, uint64_t *out_mask,
                                    ibft_wire_row_t *out_rows, int32_t *out_set, int32_t *out_vidx, ibft_tally_t *out_tally, int32_t *out_view,
                                    uint64_t *out_stored, ibft_wire_view_t *out_views, uint32_t *out_n_views, uint64_t *out_seal) {
  static_assert(IBFT_WIRE_VIEW_SEAL_RULE == wviews::SEAL_RULE, "ABI");
  const wire_views_out vo{views_cap, out_view, out_stored, out_views, out_n_views, true, out_seal};
  return wire_sets_impl(c, wire_bytes, off, n, out_mask, out_rows, out_set, out_vidx, out_tally, &vo);
}

int ibft_wire_seal_stats(ibft_ctx *c, uint32_t *commit_rows, uint32_t *seal_rows) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (commit_rows) *commit_rows = c->wire.commit_rows;
  if (seal_rows) *seal_rows = c->wire.seal_rows;
  return IBFT_OK;
}

static int wire_sets_impl(ibft_ctx *c, const uint8_t *wire_bytes, const uint32_t *off, size_t n, uint64_t *out_mask, ibft_wire_row_t *out_rows,
                          int32_t *out_set, int32_t *out_vidx, ibft_tally_t *out_tally, const wire_views_out *vo) {
  if (!c || (n && (!off || !out_mask))) return IBFT_E_INVAL;
  if (vo && n && !vo->views_cap) return IBFT_E_INVAL;
  if (!offsets_ok(off, n) || !bytes_ok(off, n, wire_bytes)) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (n > c->max_rows) return IBFT_E_TOOBIG;
  if (!c->fam.have || !c->hsets.have) return IBFT_E_NOVALSET;
  // from here to the return "the validator set" of the context is the family's union (table, size, key-cache slots)
  family_view fv(c);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  const uint32_t nr = (uint32_t)n, ns = c->fam.n_sets;
  const bool seals = vo && vo->seals;
  const uint32_t half = (nr + 63u) & ~63u;  // (seals) the seal rows begin here
  // the seal rows double the rows of the columns: grown by the first call that asks for them
  if (seals && nr && (rc = alloc_rows(c, 2 * (((uint32_t)c->max_rows + 63u) & ~63u)))) return rc;
  const size_t wbytes = n ? off[n] : 0;
  if ((rc = ensure_wire_buffers(c, wbytes))) return rc;
  if ((rc = ensure_block_records(c, c->brec, ns))) return rc;
  const uint32_t vcap = vo ? (uint32_t)std::min<size_t>(vo->views_cap, n) : 0u;  // (a cap above n behaves as n)
  const uint32_t vslots = vo && nr ? wviews::table_slots(nr, c->wviews.slots_hook) : 0u;
  if (vo && nr && (rc = ensure_wire_views(c, nr, vcap, vslots, seals))) return rc;
  if (wbytes) HIPCHK(c, hipMemcpyAsync(c->d_payload.p, wire_bytes, wbytes, hipMemcpyHostToDevice, c->stream));
  if ((rc = upload(c, c->d_off, off, (n + 1) * 4))) return rc;
  // rows judged against the union are nothing ibft_seals_launch or ibft_wire_stage_seals could re-judge under the single set
  c->staged_n = 0;
  c->staged_pre = true;
  c->wire.rows = nr;
  c->wire.columns = false;
  c->wire.begin();
  c->ev_used = 0;
  // A call that fails once kernels are enqueued may leave the tally's scratch (per-set accumulators, bitmap) half used: the map
  // goes with it, and ibft_set_height_sets — which the caller then needs again — zeroes both.
  struct map_guard {
    ibft_ctx *c;
    bool done = false;
    ~map_guard() {
      if (!done) c->hsets.have = false;
    }
  } guard{c};
  if (nr) {
    if ((rc = enqueue_wire_parse(c, nr))) return rc;
    const HeightSets &h = c->hsets;
    const ibftk::height_map m{(const uint64_t *)h.d_first.p, (const uint32_t *)h.d_range_set.p, h.n_ranges};
    hipLaunchKernelGGL(ibftk::wire_row_set_kernel, dim3((nr + 255) / 256), dim3(256), 0, c->stream, (const wire::row_info *)c->d_wire_rows.p,
                       nr, m, (int32_t *)h.d_row_set.p, (uint8_t *)c->d_pre.p);
    HIPCHK(c, hipGetLastError());
    if (seals && (rc = enqueue_wire_seals_stage(c, nr, half))) return rc;
    // (with the pre column: the seal half's tail — wavefronts whose rows are all dead — exits at once)
    if ((rc = enqueue_recover(c, c->stream, seals ? half + nr : nr, true, ibftk::MODE_SEALS, true))) return rc;
    if ((rc = enqueue_wire_sets_tally(c, nr, c->brec.map ? c->brec.map : (uint64_t *)c->brec.d.p))) return rc;
    if (seals && (rc = enqueue_wire_seals_combine(c, nr, half))) return rc;
    c->host_direct = false;
    const size_t mw = (size_t)mask_words(nr);
    if (!c->dh_mask) HIPCHK(c, hipMemcpyAsync(c->h_mask, c->d_mask_out.p, mw * 8, hipMemcpyDeviceToHost, c->stream));
    if (!c->brec.map) HIPCHK(c, hipMemcpyAsync(c->brec.h, c->brec.d.p, (size_t)ns * 32, hipMemcpyDeviceToHost, c->stream));
    if (c->cache_on) HIPCHK(c, hipMemcpyAsync(c->h_tally + 4, c->dev->d_learned.p, 8, hipMemcpyDeviceToHost, c->stream));
    if (out_rows) HIPCHK(c, hipMemcpyAsync(out_rows, c->d_wire_rows.p, n * sizeof(ibft_wire_row_t), hipMemcpyDeviceToHost, c->stream));
    if (out_set) HIPCHK(c, hipMemcpyAsync(out_set, h.d_row_set.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_vidx) HIPCHK(c, hipMemcpyAsync(out_vidx, c->d_vidx.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    uint32_t vwords[2] = {0, 0};  // {n_views, all-ones unless a table was exhausted}
    uint32_t swords[2] = {0, 0};  // (seals) {sealable rows, COMMIT rows with a set}
    if (vo) {
      WireViews &w = c->wviews;
      if ((rc = enqueue_wire_views(c, nr, vcap, vslots, seals))) return rc;
      if (seals) {
        HIPCHK(c, hipMemcpyAsync(swords, w.d_seal_words.p, 8, hipMemcpyDeviceToHost, c->stream));
        if (vo->out_seal) HIPCHK(c, hipMemcpyAsync(vo->out_seal, w.d_seal_mask.p, mw * 8, hipMemcpyDeviceToHost, c->stream));
      }
      HIPCHK(c, hipMemcpyAsync(vwords, (const uint32_t *)w.d_tables.p + 2 * (size_t)vslots, 8, hipMemcpyDeviceToHost, c->stream));
      if (vo->out_view) HIPCHK(c, hipMemcpyAsync(vo->out_view, w.d_view.p, n * 4, hipMemcpyDeviceToHost, c->stream));
      if (vo->out_stored) HIPCHK(c, hipMemcpyAsync(vo->out_stored, w.d_stored.p, mw * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->cache_on) {  // keys these rows taught the device → tables (the next call is warm)
      const uint32_t *lw = reinterpret_cast<const uint32_t *>(c->h_tally + 4);
      if ((rc = build_new_tables(c, lw[0], lw[1]))) return rc;
    }
    if (vo) {
      if (vwords[1] != 0xFFFFFFFFu) {  // (more keys than slots cannot happen: table_slots gives more slots than rows)
        c->last_error = "ibft_verify_senders_wire_views: a table was exhausted";
        return IBFT_E_HIP;
      }
      c->wviews.acc_dirty = false;  // the records kernel zeroed what the tally added
      c->wire.seal_rows = swords[0];
      c->wire.commit_rows = swords[1];
      if (vo->out_n_views) *vo->out_n_views = vwords[0];
      // the records that exist — a handful in an honest batch, where views_cap is sized for the worst — once their number is known
      const size_t filled = std::min(vwords[0], vcap);
      if (vo->out_views && filled) {
        HIPCHK(c, hipMemcpyAsync(vo->out_views, c->wviews.d_recs.p, filled * sizeof(ibft_wire_view_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
      }
    }
    memcpy(out_mask, c->h_mask, mw * 8);
    if (nr & 63) out_mask[mw - 1] &= (~0ull) >> (64 - (nr & 63));
  } else if (vo && vo->out_n_views) {
    *vo->out_n_views = 0;
  }
  fill_block_tallies(out_tally, ns, nr, c->brec.h, [&](uint32_t s) -> const uint64_t * { return &c->fam.quorum[(size_t)s * ibftk::TALLY_SUM_WORDS]; });
  c->wire.parsed = true;
  guard.done = true;
  return IBFT_OK;
}

// A batch of raw IbftMessages judged completely: the wire walk, then BOTH signatures of every message in one verdict
// launch (sender rows [0, n), seal rows [half, half + n)), the closure's hash compare folded into the combine step.
int ibft_verify_messages_wire(ibft_ctx *c, const uint8_t *wire_bytes, const uint32_t *off, size_t n, uint64_t height,
                              uint64_t round, const uint8_t *raw, size_t raw_len, uint64_t proposal_round,
                              const uint8_t *digest32, uint64_t *out_sender_mask, uint64_t *out_valid_mask,
                              uint8_t *out_class, ibft_wire_row_t *out_rows, const uint8_t *proposer20, ibft_tally_t *tally) {
  if (!c || (n && (!off || !out_sender_mask || !out_valid_mask))) return IBFT_E_INVAL;
  if ((raw_len && !raw) || raw_len > (1ull << 31)) return IBFT_E_INVAL;
  if (!offsets_ok(off, n) || !bytes_ok(off, n, wire_bytes)) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (n > c->max_rows) return IBFT_E_TOOBIG;
  if (!c->have_valset) return IBFT_E_NOVALSET;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  c->wire.columns = false;
  c->wire.begin();
  c->staged_n = 0;
  const uint32_t half = ((uint32_t)n + 63u) & ~63u;
  if ((rc = alloc_rows(c, 2 * (((uint32_t)c->max_rows + 63u) & ~63u)))) return rc;
  set_tail t;
  if ((rc = set_proposal_begin(c, digest32, raw, raw_len, proposal_round, &t.hash_needed))) return rc;
  if (n == 0) {
    if (t.hash_needed && (rc = launch_proposal_hash(c))) return rc;
    if (proposer20) {  // HasPrepareQuorum of no messages, the proposer alone: this call notes him and enqueues the tally itself
      note_proposer(c, proposer20);
      if ((rc = enqueue_tally(c, 0))) return rc;
    }
    return answer_empty_set(c, proposer20, tally);
  }
  const size_t wbytes = off[n];
  if ((rc = ensure_wire_buffers(c, wbytes))) return rc;
  if ((rc = ensure(c, c->d_noseal, c->max_rows))) return rc;
  ColumnCopies cc;
  cc.add(c->d_payload.p, wire_bytes, wbytes);
  cc.add(c->d_off.p, off, (n + 1) * 4);
  if ((rc = cc.flush(c))) return rc;
  uint8_t *d_hash = (uint8_t *)c->d_hash.p, *d_sig = (uint8_t *)c->d_sig.p, *d_signer = (uint8_t *)c->d_signer.p,
          *d_pre = (uint8_t *)c->d_pre.p;
  if ((rc = enqueue_wire_parse(c, (uint32_t)n))) return rc;
  hipLaunchKernelGGL(ibftk::wire_set_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                     (const wire::row_info *)c->d_wire_rows.p, (const uint8_t *)c->d_seal.p, (uint32_t)n, half, height, round,
                     d_hash, (uint8_t *)c->d_hash_len.p, d_sig, d_signer, d_pre, (uint8_t *)c->d_noseal.p,
                     (uint8_t *)c->d_class.p, c->dh_class);
  HIPCHK(c, hipGetLastError());
  if (half != n) {
    HIPCHK(c, hipMemsetAsync(d_sig + 65ull * n, 0, 65ull * (half - n), c->stream));
    HIPCHK(c, hipMemsetAsync(d_pre + n, 1, half - n, c->stream));
  }
  t.converted = c->seal_digest_mode != 0;
  if (t.converted && (rc = apply_seal_digest(c, d_hash + 32ull * half, (uint32_t)n, true))) return rc;
  c->ev_used = 0;
  const bool time_it = c->time_every && (c->pass_counter++ % c->time_every) == 0;
  // with the pre column: wavefronts whose rows are all dead (the seal rows of PREPAREs, other views, odd encodings) exit at once
  if ((rc = enqueue_recover(c, c->stream, half + (uint32_t)n, /*with_pre=*/true, ibftk::MODE_SEALS, time_it))) return rc;
  t.sender_pre = d_pre;  // not canonical here, or From / Signature of a length no signature check can pass
  t.valid_pre = d_pre + half;
  t.no_seal = (const uint8_t *)c->d_noseal.p;
  t.half_words = half / 64;
  t.note_proposer = true;
  t.proposer20 = proposer20;
  if ((rc = enqueue_set_tally(c, n, half, t))) return rc;
  if (out_class && !c->dh_class)
    HIPCHK(c, hipMemcpyAsync(c->h_class, c->d_class.p, n, hipMemcpyDeviceToHost, c->stream));
  if (out_rows)  // 80 B per row through a copy command: ask for it only when the fields are needed (out_class routes)
    HIPCHK(c, hipMemcpyAsync(out_rows, c->d_wire_rows.p, n * sizeof(ibft_wire_row_t), hipMemcpyDeviceToHost, c->stream));
  if ((rc = fetch_set_masks(c, n, out_sender_mask, out_valid_mask, tally))) return rc;
  if (out_class) memcpy(out_class, c->h_class, n);
  c->wire.rows = (uint32_t)n;
  c->wire.parsed = true;
  return IBFT_OK;
}

// §8f rank 2 from the transport's bytes: the whole certificate tree of a batch of PREPREPARE / ROUND_CHANGE messages —
// every nested message a row — expanded level by level on the device (kernels.hip.h: cert_*_kernel), then ONE verdict
// launch over all rows.  The host takes part once per level: it reads the next level's row count to size the launches.
//
// judge (ibft_judge_certificates_wire): the same path, then one record per carrier — validPC and the RoundChangeCertificate rules
// (cert_verdict_dev.h) over the rows where they lie (kernels.hip.h: cert_judge_kernel); every per-row output is optional then.
//
// The call runs as stages over one cert_call (what the caller gave) and one cert_plan (what the stages found out), in this
// order: cert_check, cert_reserve, cert_expand, cert_digests, cert_verdicts, cert_compare_and_judge, cert_decide, cert_deliver.
//
// decide (ibft_decide_certificates_wire): the judge path, then one decision per record under the proposer table of
// ibft_set_proposers (cert_decide_dev.h; kernels.hip.h: cert_decide_records_kernel, cert_decide_proposals_kernel).
struct cert_call {
  const uint8_t *wire_bytes;
  const uint32_t *off;
  size_t n, rows_cap, certs_cap;  // certs_cap: judge only
  bool judge, decide;                // decide: judge, and out_decision[i] next to out_cert[i]
  size_t *out_n_rows, *out_n_certs;  // out_n_certs, out_cert: judge only
  ibft_cert_verdict_t *out_cert;
  ibft_cert_decision_t *out_decision;
  ibft_cert_node_t *out_nodes;  // every per-row output may be null (out_sender_mask: with judge only)
  ibft_wire_row_t *out_rows;
  uint8_t *out_class;
  uint64_t *out_sender_mask, *out_hash_mask, *out_self_mask;
  // ibft_decide_round_changes_wire: decide, and the quorum records of the level-0 ROUND_CHANGE rows with the answer to `query`
  bool round_changes;
  const ibft_rc_query_t *query;  // null: no answer
  size_t rc_cap;
  int32_t *out_rc_view;          // may be null, as out_rc_stored and out_answer
  uint64_t *out_rc_stored;
  ibft_rc_record_t *out_rc;
  size_t *out_n_rc;
  ibft_rc_answer_t *out_answer;
};
struct cert_plan {
  uint32_t rc_cap = 0, rc_slots = 0;                   // round changes: min(n, rc_cap), slots of each table
  size_t cap = 0;                                      // rows the tree may have: min(rows_cap, max_rows)
  std::vector<std::pair<uint32_t, uint32_t>> levels;   // rows [first, second) of each level
  uint32_t rows = 0, carriers = 0, records = 0;        // of the whole tree; carriers: the deferred rows (slot list)
  bool two = false;                                    // the deferred rows get a verdict launch of their own …
  uint32_t region = 0;                                 // … as rows [region, region + carriers) of the columns
  uint32_t dense_base = 0;                             // the dedup's dense batch begins here
  uint8_t *d_digest = nullptr, *d_sig = nullptr, *d_from = nullptr, *d_pre = nullptr;  // the shared columns
  void read_columns(const ibft_ctx *c) {  // again after every alloc_rows: the columns may have moved
    d_digest = (uint8_t *)c->d_hash.p, d_sig = (uint8_t *)c->d_sig.p, d_from = (uint8_t *)c->d_signer.p, d_pre = (uint8_t *)c->d_pre.p;
  }
};
constexpr int CERT_NOTHING_TO_DO = 1;  // cert_check: a batch without rows is answered already

// What can be refused.  locked = false: the arguments, before the context's lock is taken (c may be null); the counts are
// zeroed once the arguments stand.  locked = true: against the context — size, validator set, the empty batch, the records' room.
static int cert_check(const ibft_ctx *c, const cert_call &k, cert_plan &p, bool locked) {
  if (!locked) {
    if (!c || !k.out_n_rows || (k.n && (!k.off || (!k.judge && !k.out_sender_mask)))) return IBFT_E_INVAL;
    if (k.judge && (!k.out_n_certs || (k.n && !k.out_cert))) return IBFT_E_INVAL;
    if (k.decide && k.n && !k.out_decision) return IBFT_E_INVAL;
    if (k.round_changes && (!k.out_n_rc || (k.n && (!k.out_rc || !k.rc_cap)))) return IBFT_E_INVAL;
    if (k.round_changes && k.query && (k.query->has_accepted_proposal > 1 || k.query->reserved)) return IBFT_E_INVAL;
    if (!offsets_ok(k.off, k.n) || !bytes_ok(k.off, k.n, k.wire_bytes)) return IBFT_E_INVAL;
    *k.out_n_rows = 0;
    if (k.judge) *k.out_n_certs = 0;
    if (k.round_changes) *k.out_n_rc = 0;
    return IBFT_OK;
  }
  p.cap = std::min<size_t>(k.rows_cap, c->max_rows);
  if (k.n > p.cap) return IBFT_E_TOOBIG;
  if (!c->have_valset) return IBFT_E_NOVALSET;
  if (k.n == 0) return CERT_NOTHING_TO_DO;
  if (k.judge && k.n > k.certs_cap) return IBFT_E_TOOBIG;
  return IBFT_OK;
}

// every buffer, the pinned counter block and the two events the call may need, and the rows of the columns
static int cert_reserve(ibft_ctx *c, const cert_call &k, cert_plan &p) {
  CertState &s = c->cert;
  int rc;
  const size_t wbytes = k.off[k.n], m = c->max_rows;
  if ((rc = ensure(c, c->d_payload, wbytes + 256))) return rc;
  if ((rc = ensure(c, c->d_wire_rows, m * sizeof(wire::row_info)))) return rc;
  c->wire.begin();  // the tree's rows take the place of the last flat call's
  if ((rc = ensure(c, s.nodes, m * sizeof(wire::node_info)))) return rc;
  if ((rc = ensure(c, s.span, m * 8))) return rc;
  if ((rc = ensure(c, s.count, m * 4))) return rc;
  if ((rc = ensure(c, s.slot, m * 4))) return rc;
  if ((rc = ensure(c, s.prop, m * 32))) return rc;
  if ((rc = ensure(c, s.masks, (size_t)mask_words(m) * 16))) return rc;
  const bool fresh_total = !s.total.p;
  if ((rc = ensure(c, s.total, sizeof(cert_counters)))) return rc;
  if (fresh_total) HIPCHK(c, hipMemset(s.total.p, 0, sizeof(cert_counters)));  // (count_acc: zero between launches)
  if ((rc = ensure(c, s.tiles, (m / 1024 + 2) * 8))) return rc;
  const uint32_t dd_slots = s.dedup ? cdd::table_slots((uint32_t)m, s.dedup_slots_cap) : 0u;
  if (s.dedup && (rc = ensure(c, s.dd_table, (size_t)dd_slots * 4))) return rc;
  if (s.dedup && (rc = ensure(c, s.dd_slot, m * 4))) return rc;
  if (s.dedup && (rc = ensure(c, s.dd_pos, m * 4))) return rc;
  if (k.judge && (rc = ensure(c, s.rec, m * sizeof(certv::record)))) return rc;
  if (k.judge && (rc = ensure(c, s.recbase, (m + 1) * 4))) return rc;
  if (k.decide && (rc = ensure(c, s.dec, m * sizeof(certd::decision)))) return rc;
  if (k.decide && (rc = ensure(c, s.mid, k.n * 25 * sizeof(uint64_t)))) return rc;
  if (k.round_changes) {
    const uint32_t n = (uint32_t)k.n;
    p.rc_cap = (uint32_t)std::min<size_t>(k.rc_cap, k.n);  // (a cap above n behaves as n)
    p.rc_slots = wviews::table_slots(n, s.rc_slots_hook);
    const size_t acc_bytes = (size_t)p.rc_cap * rcd::acc_words(2 * (int)c->power_words) * 8;
    if (acc_bytes > s.rc_acc.cap) s.rc_acc_dirty = true;  // a fresh allocation holds anything
    if ((rc = ensure(c, s.rc_tables, (size_t)p.rc_slots * 8 + 16)) || (rc = ensure(c, s.rc_slots, (size_t)n * 8)) ||
        (rc = ensure(c, s.rc_vidx, (size_t)n * 4)) || (rc = ensure(c, s.rc_rank, (size_t)n * 4)) || (rc = ensure(c, s.rc_first, (size_t)p.rc_cap * 4)) ||
        (rc = ensure(c, s.rc_view, (size_t)n * 4)) || (rc = ensure(c, s.rc_stored, (size_t)mask_words(n) * 8)) || (rc = ensure(c, s.rc_acc, acc_bytes)) ||
        (rc = ensure(c, s.rc_recs, (size_t)p.rc_cap * sizeof(rcd::record))) || (rc = ensure(c, s.rc_answer, sizeof(rcd::answer))))
      return rc;
  }
  if (!s.h_total) {
    if (hipHostMalloc((void **)&s.h_total, sizeof(cert_counters)) != hipSuccess) return IBFT_E_NOMEM;
    void *d = nullptr;
    if (!getenv("IBFT_NO_HOST_DIRECT") && hipHostGetDevicePointer(&d, s.h_total, 0) == hipSuccess) s.dh_total = (cert_counters *)d;
  }
  if (!s.ev_fork) {
    HIPCHK(c, hipEventCreateWithFlags(&s.ev_fork, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&s.ev_join, hipEventDisableTiming));
  }
  // the columns hold the tree's rows and, with two verdict launches, the batch of the deferred rows behind them (64-aligned);
  // with the dedup, the dense batch of the representatives behind both
  const uint32_t rows_al = ((uint32_t)c->max_rows + 63u) & ~63u;
  if ((s.overlap || s.dedup) && (rc = alloc_rows(c, (s.dedup ? 3u : 2u) * rows_al))) return rc;
  p.read_columns(c);
  return IBFT_OK;
}

// The bytes and level 0 go up; then level by level: parse, count the children, scan (the host reads the next level's size),
// list them.  With judge, the records are counted while level 1 is listed.  → p.levels, p.rows, p.carriers, p.records
static int cert_expand(ibft_ctx *c, const cert_call &k, cert_plan &p) {
  CertState &s = c->cert;
  const size_t n = k.n, wbytes = k.off[n];
  const uint8_t *d_wire = (const uint8_t *)c->d_payload.p;
  wire::node_info *d_nodes = (wire::node_info *)s.nodes.p;
  wire::row_info *d_rows = (wire::row_info *)c->d_wire_rows.p;
  uint2 *d_span = (uint2 *)s.span.p;
  uint32_t *d_count = (uint32_t *)s.count.p, *d_slot = (uint32_t *)s.slot.p;
  cert_counters *d_total = (cert_counters *)s.total.p;
  const volatile cert_counters *h_total = s.h_total;
  if (wbytes) HIPCHK(c, hipMemcpyAsync(c->d_payload.p, k.wire_bytes, wbytes, hipMemcpyHostToDevice, c->stream));
  std::vector<wire::node_info> level0(n);
  for (size_t i = 0; i < n; i++) {
    wire::node_info nd{};
    nd.off = k.off[i];
    nd.len = k.off[i + 1] - k.off[i];
    nd.parent = wire::NO_PARENT;
    nd.ordinal = (uint32_t)i;
    nd.role = wire::ROLE_ROOT;
    level0[i] = nd;
  }
  HIPCHK(c, hipMemcpyAsync(d_nodes, level0.data(), n * sizeof(wire::node_info), hipMemcpyHostToDevice, c->stream));
  uint32_t lo = 0, hi = (uint32_t)n, carriers = 0;
  for (uint32_t level = 0;; level++) {
    const uint32_t cnt = hi - lo;
    hipLaunchKernelGGL(ibftk::cert_parse_kernel, dim3((cnt + 63) / 64), dim3(64), 0, c->stream, d_wire, d_nodes, lo, hi, d_rows, d_span,
                       p.d_digest, p.d_sig, p.d_from, p.d_pre);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(ibftk::cert_walk_kernel<false>, dim3(cnt), dim3(64), 0, c->stream, d_wire, d_nodes, d_rows, (const uint2 *)d_span, lo, hi,
                       d_count);
    HIPCHK(c, hipGetLastError());
    ibftk::cert_scan_launch(c->stream, cnt <= ibftk::CERT_SCAN_ONE_GROUP_MAX, (const uint32_t *)d_count, d_nodes, lo, cnt, hi, carriers, d_slot,
                            (uint2 *)s.tiles.p, &d_total->next_rows, s.dh_total ? &s.dh_total->next_rows : nullptr);
    HIPCHK(c, hipGetLastError());
    // next_rows and carriers; behind level 1 of a judge call also the records its listing counted
    const size_t scan_bytes = k.judge && level == 1 ? offsetof(cert_counters, pad0) : offsetof(cert_counters, records);
    if (!s.dh_total) HIPCHK(c, hipMemcpyAsync(s.h_total, d_total, scan_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    p.levels.push_back({lo, hi});
    const uint32_t total = h_total->next_rows;
    carriers += h_total->carriers;
    if (total == 0) break;
    if ((uint64_t)hi + total > p.cap || level == 254) return IBFT_E_TOOBIG;
    hipLaunchKernelGGL(ibftk::cert_walk_kernel<true>, dim3(cnt), dim3(64), 0, c->stream, d_wire, d_nodes, d_rows, (const uint2 *)d_span, lo, hi,
                       d_count);
    HIPCHK(c, hipGetLastError());
    lo = hi;
    hi += total;
    // level 1 is listed: which of its rows get a record (the kernel is handed the block and writes its word 2, `records`; the next
    // level's synchronisation delivers it)
    if (k.judge && level == 0) {
      hipLaunchKernelGGL(ibftk::cert_record_scan_kernel, dim3(1), dim3(1024), 0, c->stream, (const wire::node_info *)d_nodes, (uint32_t)n, hi,
                         (uint32_t *)s.recbase.p, &d_total->next_rows, s.dh_total ? &s.dh_total->next_rows : nullptr);
      HIPCHK(c, hipGetLastError());
    }
  }
  p.rows = hi;
  p.carriers = carriers;
  // records: every level-0 row, every level-1 row of a RoundChangeCertificate
  p.records = k.judge ? (p.levels.size() > 1 ? h_total->records : (uint32_t)n) : 0u;
  if (k.judge && (p.records < n || p.records > p.rows)) {
    c->last_error = "certificate records: a count outside [n, rows]";
    return IBFT_E_HIP;
  }
  if (k.judge && p.records > k.certs_cap) return IBFT_E_TOOBIG;
  return IBFT_OK;
}

// What the parents know goes down the levels; then the rows' digests: the proposal digests cleared, the deferred digests a
// wavefront each, the rest by cert_finish_kernel — on the side stream when the deferred rows get a verdict launch of their own
// (→ p.two, p.region), which the carrier stage then fills; the join event is left for cert_verdicts to wait on.
static int cert_digests(ibft_ctx *c, const cert_call &k, cert_plan &p) {
  CertState &s = c->cert;
  int rc;
  const uint8_t *d_wire = (const uint8_t *)c->d_payload.p;
  wire::node_info *d_nodes = (wire::node_info *)s.nodes.p;
  wire::row_info *d_rows = (wire::row_info *)c->d_wire_rows.p;
  const uint32_t *d_slot = (const uint32_t *)s.slot.p;
  uint8_t *d_prop = (uint8_t *)s.prop.p;
  const uint32_t rows = p.rows, carriers = p.carriers;
  for (size_t l = p.levels.size(); l-- > 1;) {
    const uint32_t cnt = p.levels[l].second - p.levels[l].first;
    hipLaunchKernelGGL(ibftk::cert_propagate_kernel, dim3((cnt + 255) / 256), dim3(256), 0, c->stream, (const wire::node_info *)d_nodes, d_rows,
                       p.levels[l].first, p.levels[l].second);
    HIPCHK(c, hipGetLastError());
  }
  // The deferred digests (messages that carry certificates, long messages) — a wavefront per message, a sequential sponge each — run
  // on the side stream NEXT TO the verdict launch over all the other rows; the deferred rows then get a small verdict launch of their
  // own as rows [region, region + carriers) of the columns.  That pays when the verdict launch is in its throughput regime (many
  // wavefronts per SIMD: ≥ 4 096 rows, or the known-key kernels): N = 1 024 cold 20.7 → 17.8 ms, warm 12.3 → 10.1; N = 256 warm
  // 2.04 → 1.89.  A small cold launch is one wavefront per SIMD whose duration is its slowest wavefront, and a wavefront that shares
  // its SIMD with a digest wavefront runs at ≈55 % speed (N = 64 cold 1.08 → 1.12 ms): one stream, one verdict launch there.
  // IBFT_CERT_OVERLAP=0: never.
  p.two = s.overlap && carriers != 0 && (rows >= 4096u || (c->cache_on && c->my_built > 0));
  p.region = p.two ? ((rows + 63u) & ~63u) : 0u;
  hipStream_t ds = p.two ? c->hstream : c->stream;
  if (p.two) {
    if ((rc = alloc_rows(c, 2 * (((uint32_t)c->max_rows + 63u) & ~63u)))) return rc;
    p.read_columns(c);
    HIPCHK(c, hipEventRecord(s.ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(ds, s.ev_fork, 0));
  }
  HIPCHK(c, hipMemsetAsync(d_prop, 0, (size_t)rows * 32, ds));  // rows without a Proposal: a zero digest (cert_finish_kernel skips them)
  if (carriers) {
    hipLaunchKernelGGL(ibftk::cert_digest_wave_kernel, dim3(2 * carriers), dim3(64), 0, ds, d_wire, (const wire::node_info *)d_nodes,
                       (const wire::row_info *)d_rows, d_slot, p.region, p.d_digest, d_prop, k.decide ? (uint64_t *)s.mid.p : (uint64_t *)nullptr,
                       k.decide ? (uint32_t)k.n : 0u);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(ibftk::cert_finish_kernel, dim3((rows + 63) / 64), dim3(64), 0, ds, d_wire, d_nodes, (const wire::row_info *)d_rows, rows,
                     p.d_digest, d_prop, p.d_pre, p.two ? 1u : 0u);
  HIPCHK(c, hipGetLastError());
  if (p.two) {
    hipLaunchKernelGGL(ibftk::cert_carrier_stage_kernel, dim3((carriers + 255) / 256), dim3(256), 0, ds, (const wire::node_info *)d_nodes,
                       (const wire::row_info *)d_rows, d_slot, carriers, p.region, p.d_sig, p.d_from, p.d_pre);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(s.ev_join, ds));
  }
  return IBFT_OK;
}

// The verdict launch over all rows of all levels: the digest column holds keccak256(PayloadNoSig) — the seal-style pass; rows that
// are not judged here (and, with two launches, the deferred rows) are pre-flagged.  Plain, or through the dedup; then the deferred
// batch's launch and scatter; then the count of what was judged (ibft_cert_stats).
static int cert_verdicts(ibft_ctx *c, const cert_call &, cert_plan &p) {
  CertState &s = c->cert;
  int rc;
  cert_counters *d_total = (cert_counters *)s.total.p;
  const volatile cert_counters *h_total = s.h_total;
  const uint32_t rows = p.rows, carriers = p.carriers, region = p.region;
  c->ev_used = 0;
  if (!s.dedup) {
    if ((rc = enqueue_recover(c, c->stream, rows, true, ibftk::MODE_SEALS, false))) return rc;
  } else {
    // The same verdicts from one launch over the distinct (digest, signature, From) of the rows without a pre-flag
    // (cert_dedup_dev.h): table, representatives, their dense batch behind the tree's rows and the deferred batch, its
    // verdict launch (the AUTO rule and learn_key see the dense batch), every row its representative's bit.
    const uint32_t slots = cdd::table_slots(rows, s.dedup_slots_cap);
    p.dense_base = p.two ? ((region + carriers + 63u) & ~63u) : ((rows + 63u) & ~63u);
    uint32_t *d_table = (uint32_t *)s.dd_table.p, *d_dd_slot = (uint32_t *)s.dd_slot.p, *d_dd_pos = (uint32_t *)s.dd_pos.p;
    const cdd::columns cols{p.d_digest, p.d_sig, p.d_from, p.d_pre};
    // with kernel timing on, two event pairs: table + compaction, scatter (the verdict launch between them is not timed on this
    // path) — ibft_last_kernel_ms after a flag-on ibft_verify_certificates_wire is the time of the dedup's own kernels
    hipEvent_t t0 = nullptr, t1 = nullptr, t2 = nullptr, t3 = nullptr;
    if (c->time_every && ((rc = next_events(c, &t0, &t1)) || (rc = next_events(c, &t2, &t3)))) return rc;
    if (t0) HIPCHK(c, hipEventRecord(t0, c->stream));
    HIPCHK(c, ibftk::cert_dedup_front_launch(c->stream, cols, rows, slots, p.dense_base, d_table, d_dd_slot, (uint32_t *)s.count.p, (uint2 *)s.tiles.p,
                                             d_dd_pos, &d_total->dense, s.dh_total ? &s.dh_total->dense : nullptr));
    HIPCHK(c, hipGetLastError());
    if (t1) HIPCHK(c, hipEventRecord(t1, c->stream));
    if (!s.dh_total)  // dense, unplaced
      HIPCHK(c, hipMemcpyAsync(&s.h_total->dense, &d_total->dense, offsetof(cert_counters, judged_tree) - offsetof(cert_counters, dense),
                               hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t dense = h_total->dense;
    if (dense > rows) {
      c->last_error = "certificate dedup: more representatives than rows";
      return IBFT_E_HIP;
    }
    uint64_t *d_dense_mask = (uint64_t *)c->d_mask.p + p.dense_base / 64;
    // the dense batch's verdict words: zero whatever an earlier call left there; the tree's own words are stored whole below
    if (dense) HIPCHK(c, hipMemsetAsync(d_dense_mask, 0, (size_t)mask_words(dense) * 8, c->stream));
    if ((rc = enqueue_recover(c, c->stream, dense, true, ibftk::MODE_SEALS, false, p.dense_base, true))) return rc;
    if (t2) HIPCHK(c, hipEventRecord(t2, c->stream));
    ibftk::cert_dedup_scatter_launch(c->stream, (const uint32_t *)d_table, (const uint32_t *)d_dd_slot, (const uint32_t *)d_dd_pos,
                                     (const uint64_t *)d_dense_mask, rows, (uint64_t *)c->d_mask.p);
    HIPCHK(c, hipGetLastError());
    if (t3) HIPCHK(c, hipEventRecord(t3, c->stream));
    c->mask_dirty_words = std::max(c->mask_dirty_words, (uint32_t)mask_words(rows));
  }
  if (p.two) {
    HIPCHK(c, hipStreamWaitEvent(c->stream, s.ev_join, 0));
    // the deferred rows' verdict words: zero whatever an earlier call left there (the first launch only vouches for its own words)
    HIPCHK(c, hipMemsetAsync((uint64_t *)c->d_mask.p + region / 64, 0, (size_t)mask_words(carriers) * 8, c->stream));
    if ((rc = enqueue_recover(c, c->stream, carriers, true, ibftk::MODE_SEALS, false, region, true))) return rc;
    hipLaunchKernelGGL(ibftk::cert_scatter_kernel, dim3((carriers + 255) / 256), dim3(256), 0, c->stream, (const uint32_t *)s.slot.p, carriers, region,
                       (uint64_t *)c->d_mask.p);
    HIPCHK(c, hipGetLastError());
  }
  // ibft_cert_stats: how many rows the verdict launches judged (no pre-flag), the tree's rows and the deferred batch apart
  ibftk::cert_dedup_count_launch(c->stream, (const uint8_t *)p.d_pre, rows, (const uint8_t *)p.d_pre + region, p.two ? carriers : 0u, d_total->count_acc,
                                 &d_total->judged_tree, s.dh_total ? &s.dh_total->judged_tree : nullptr);
  HIPCHK(c, hipGetLastError());
  if (!s.dh_total)  // judged_tree, judged_deferred
    HIPCHK(c, hipMemcpyAsync(&s.h_total->judged_tree, &d_total->judged_tree, offsetof(cert_counters, count_acc) - offsetof(cert_counters, judged_tree),
                             hipMemcpyDeviceToHost, c->stream));
  return IBFT_OK;
}

// every row's hash / self words and class byte; with judge, one record per carrier over them and their way home
static int cert_compare_and_judge(ibft_ctx *c, const cert_call &k, cert_plan &p) {
  CertState &s = c->cert;
  int rc;
  const size_t n = k.n;
  wire::node_info *d_nodes = (wire::node_info *)s.nodes.p;
  wire::row_info *d_rows = (wire::row_info *)c->d_wire_rows.p;
  uint64_t *d_hash_mask = (uint64_t *)s.masks.p, *d_self_mask = d_hash_mask + mask_words(c->max_rows);
  hipLaunchKernelGGL(ibftk::cert_compare_kernel, dim3((p.rows + 255) / 256), dim3(256), 0, c->stream, (const wire::node_info *)d_nodes,
                     (const wire::row_info *)d_rows, (const uint8_t *)s.prop.p, p.rows, d_hash_mask, d_self_mask, (uint8_t *)c->d_class.p);
  HIPCHK(c, hipGetLastError());
  if (!k.judge) return IBFT_OK;
  ibftk::cert_judge_args ja{};
  ja.nodes = d_nodes;
  ja.rows = d_rows;
  ja.cls = (const uint8_t *)c->d_class.p;
  ja.sender_mask = (const uint64_t *)c->d_mask.p;
  ja.hash_mask = d_hash_mask;
  ja.self_mask = d_self_mask;
  ja.vtab = (const uint32_t *)c->d_vtab.p;
  ja.vpower32 = (const uint32_t *)c->d_vpower.p;
  ja.quorum = (const uint64_t *)c->d_quorum.p;
  ja.rec_base = p.levels.size() > 1 ? (const uint32_t *)s.recbase.p : nullptr;
  ja.vslot_mask = c->vslot_mask;
  ja.n_validators = c->n_validators;
  ja.n_roots = (uint32_t)n;
  ja.n_rows = p.rows;
  ja.n_records = p.records;
  size_t dyn;
  ja.lds_bitmap = bitmap_in_lds(c->n_validators, &dyn);  // 0: one workgroup walks every record over the HBM bitmap
  ja.seen = (uint32_t *)c->d_seen.p;
  ja.out = (certv::record *)s.rec.p;
  const dim3 grid(ja.lds_bitmap ? std::min(p.records, ibftk::CERT_JUDGE_MAX_GRID) : 1u);
  // (the verdict launches of this path are not timed: with kernel timing on, ibft_last_kernel_ms after this call is the two
  // record kernels' time)
  hipEvent_t j0 = nullptr, j1 = nullptr;
  if (c->time_every) {
    if ((rc = next_events(c, &j0, &j1))) return rc;
    HIPCHK(c, hipEventRecord(j0, c->stream));
  }
  with_power_words(c->power_words, [&](auto PW) { hipLaunchKernelGGL(ibftk::cert_judge_kernel<decltype(PW)::value>, grid, dim3(64), dyn, c->stream, ja); });
  HIPCHK(c, hipGetLastError());
  if (ja.rec_base) {
    hipLaunchKernelGGL(ibftk::cert_judge_children_kernel, dim3(std::min((uint32_t)n, ibftk::CERT_JUDGE_MAX_GRID)), dim3(64), 0, c->stream, ja.out,
                       (uint32_t)n);
    HIPCHK(c, hipGetLastError());
  }
  if (j1) HIPCHK(c, hipEventRecord(j1, c->stream));
  HIPCHK(c, hipMemcpyAsync(k.out_cert, ja.out, (size_t)p.records * sizeof(certv::record), hipMemcpyDeviceToHost, c->stream));
  return IBFT_OK;
}

// decide: behind the records, one decision per record and its way home.  (With kernel timing on, the two launches get an event
// pair of their own: ibft_last_kernel_ms after this call is the record kernels' time plus theirs.)
static int cert_decide(ibft_ctx *c, const cert_call &k, cert_plan &p) {
  if (!k.decide) return IBFT_OK;
  CertState &s = c->cert;
  int rc;
  ibftk::cert_decide_args da{};
  da.nodes = (const wire::node_info *)s.nodes.p;
  da.rows = (const wire::row_info *)c->d_wire_rows.p;
  da.rec = (const certv::record *)s.rec.p;
  da.wire_bytes = (const uint8_t *)c->d_payload.p;
  da.mid_state = (const uint64_t *)s.mid.p;
  da.table = certd::proposer_table{s.prop_height, s.prop_first, (const uint8_t *)s.proposers.p, s.proposers.p ? s.prop_rounds : 0u};
  da.n_roots = (uint32_t)k.n;
  da.n_rows = p.rows;
  da.n_records = p.records;
  da.out = (certd::decision *)s.dec.p;
  hipEvent_t d0 = nullptr, d1 = nullptr;
  if (c->time_every) {
    if ((rc = next_events(c, &d0, &d1))) return rc;
    HIPCHK(c, hipEventRecord(d0, c->stream));
  }
  hipLaunchKernelGGL(ibftk::cert_decide_records_kernel, dim3((p.records + 255) / 256), dim3(256), 0, c->stream, da);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(ibftk::cert_decide_proposals_kernel, dim3(std::min((uint32_t)k.n, ibftk::CERT_JUDGE_MAX_GRID)), dim3(64), 0, c->stream, da);
  HIPCHK(c, hipGetLastError());
  if (d1) HIPCHK(c, hipEventRecord(d1, c->stream));
  HIPCHK(c, hipMemcpyAsync(k.out_decision, da.out, (size_t)p.records * sizeof(certd::decision), hipMemcpyDeviceToHost, c->stream));
  return IBFT_OK;
}

// round changes: behind the decisions, one fill (tables to EMPTY, the call's words to all-ones), then index, insert, rank, tally,
// records and — with a query — select, and their way home.  No host wait: the three words leave with what cert_deliver waits for.
static int cert_round_changes(ibft_ctx *c, const cert_call &k, cert_plan &p) {
  if (!k.round_changes) return IBFT_OK;
  CertState &s = c->cert;
  const uint32_t n = (uint32_t)k.n, slots = p.rc_slots;
  if (s.rc_acc_dirty) HIPCHK(c, hipMemsetAsync(s.rc_acc.p, 0, s.rc_acc.cap, c->stream));
  s.rc_acc_dirty = true;  // until this call has come back clean
  HIPCHK(c, hipMemsetAsync(s.rc_tables.p, 0xFF, (size_t)slots * 8 + 16, c->stream));
  ibftk::round_change_args a{};
  a.rows = (const wire::row_info *)c->d_wire_rows.p;
  a.rec = (const certv::record *)s.rec.p;
  a.dec = (const certd::decision *)s.dec.p;
  a.vtab = (const uint32_t *)c->d_vtab.p;
  a.vpower32 = (const uint32_t *)c->d_vpower.p;
  a.quorum = (const uint64_t *)c->d_quorum.p;
  a.vslot_mask = c->vslot_mask;
  a.n_validators = c->n_validators;
  a.n = n;
  a.cap = p.rc_cap;
  a.slots = slots;
  a.salt = c->wviews.salt;
  a.n_pieces = 2 * (int)c->power_words;
  a.vidx = (int32_t *)s.rc_vidx.p;
  a.key_table = (uint32_t *)s.rc_tables.p;
  a.last_table = a.key_table + slots;
  a.slot_key = (uint32_t *)s.rc_slots.p;
  a.slot_last = a.slot_key + n;
  a.rank_of = (uint32_t *)s.rc_rank.p;
  a.first_row = (uint32_t *)s.rc_first.p;
  a.words = a.key_table + 2 * (size_t)slots;
  a.out_view = (int32_t *)s.rc_view.p;
  a.out_stored = (uint64_t *)s.rc_stored.p;
  a.acc = (uint64_t *)s.rc_acc.p;
  a.out_rc = (rcd::record *)s.rc_recs.p;
  a.out_answer = (rcd::answer *)s.rc_answer.p;
  const bool ask = k.query && k.out_answer;
  if (ask) a.query = rcd::query{k.query->height, k.query->round, k.query->min_round, k.query->has_accepted_proposal, 0u};
  const dim3 rows_grid((n + ibftk::RC_THREADS - 1) / ibftk::RC_THREADS), block(ibftk::RC_THREADS);
  hipLaunchKernelGGL(ibftk::round_change_index_kernel, rows_grid, block, 0, c->stream, a);
  hipLaunchKernelGGL(ibftk::round_change_insert_kernel, rows_grid, block, 0, c->stream, a);
  hipLaunchKernelGGL(ibftk::round_change_rank_kernel, dim3(1), dim3(1024), 0, c->stream, a);
  with_power_words(c->power_words,
                   [&](auto PW) { hipLaunchKernelGGL(ibftk::round_change_tally_kernel<decltype(PW)::value>, rows_grid, block, 0, c->stream, a); });
  hipLaunchKernelGGL(ibftk::round_change_records_kernel, dim3((p.rc_cap + ibftk::RC_THREADS - 1) / ibftk::RC_THREADS), block, 0, c->stream, a);
  if (ask) hipLaunchKernelGGL(ibftk::round_change_select_kernel, dim3(1), dim3(64), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  // (into the pinned counter block, which outlives a call that returns early, not into this call's frame)
  HIPCHK(c, hipMemcpyAsync(s.h_total->rc_words, a.words, sizeof s.h_total->rc_words, hipMemcpyDeviceToHost, c->stream));
  if (k.out_rc_view) HIPCHK(c, hipMemcpyAsync(k.out_rc_view, a.out_view, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (k.out_rc_stored) HIPCHK(c, hipMemcpyAsync(k.out_rc_stored, a.out_stored, (size_t)mask_words(n) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(k.out_rc, a.out_rc, (size_t)p.rc_cap * sizeof(rcd::record), hipMemcpyDeviceToHost, c->stream));
  if (ask) HIPCHK(c, hipMemcpyAsync(k.out_answer, a.out_answer, sizeof(rcd::answer), hipMemcpyDeviceToHost, c->stream));
  return IBFT_OK;
}

// the per-row outputs that were asked for, the sender words (fetch_results waits for the stream), the counts, the stats
static int cert_deliver(ibft_ctx *c, const cert_call &k, cert_plan &p) {
  CertState &s = c->cert;
  int rc;
  const uint32_t rows = p.rows;
  const uint64_t *d_hash_mask = (const uint64_t *)s.masks.p, *d_self_mask = d_hash_mask + mask_words(c->max_rows);
  const size_t mw = (size_t)mask_words(rows);
  if (k.out_nodes) HIPCHK(c, hipMemcpyAsync(k.out_nodes, s.nodes.p, (size_t)rows * sizeof(wire::node_info), hipMemcpyDeviceToHost, c->stream));
  if (k.out_rows) HIPCHK(c, hipMemcpyAsync(k.out_rows, c->d_wire_rows.p, (size_t)rows * sizeof(wire::row_info), hipMemcpyDeviceToHost, c->stream));
  if (k.out_class) HIPCHK(c, hipMemcpyAsync(k.out_class, c->d_class.p, rows, hipMemcpyDeviceToHost, c->stream));
  if (k.out_hash_mask) HIPCHK(c, hipMemcpyAsync(k.out_hash_mask, d_hash_mask, mw * 8, hipMemcpyDeviceToHost, c->stream));
  if (k.out_self_mask) HIPCHK(c, hipMemcpyAsync(k.out_self_mask, d_self_mask, mw * 8, hipMemcpyDeviceToHost, c->stream));
  // no tally: the rows of a tree belong to many certificates; their quorum rules are the caller's (From / type / view columns)
  if ((rc = fetch_results(c, rows, k.out_sender_mask, nullptr, false))) return rc;
  if (k.round_changes) {
    const volatile cert_counters *hw = s.h_total;
    if (hw->rc_words[1] != 0xFFFFFFFFu) {  // (more keys than slots cannot happen: table_slots gives more slots than rows)
      c->last_error = "ibft_decide_round_changes_wire: a table was exhausted";
      return IBFT_E_HIP;
    }
    s.rc_acc_dirty = false;  // the records kernel zeroed what the tally added
    *k.out_n_rc = hw->rc_words[0];
  }
  *k.out_n_rows = rows;
  if (k.judge) *k.out_n_certs = p.records;
  const volatile cert_counters *h = s.h_total;
  const uint32_t judged = h->judged_tree + h->judged_deferred;
  s.stat[0] = rows;
  s.stat[1] = judged;
  s.stat[2] = s.dedup ? h->dense + h->judged_deferred : judged;
  s.stat[3] = s.dedup ? h->unplaced : 0u;
  return IBFT_OK;
}

static int certificates_wire_impl(ibft_ctx *c, const cert_call &k) {
  static_assert(sizeof(ibft_cert_node_t) == sizeof(wire::node_info), "ABI");
  static_assert(IBFT_CERT_DIGEST_MAX_BYTES == wire::TREE_DIGEST_MAX_BYTES, "ABI");
  static_assert(sizeof(ibft_cert_verdict_t) == sizeof(certv::record) && sizeof(ibft_cert_verdict_t) == 128, "ABI");
  static_assert(offsetof(ibft_cert_verdict_t, pc) == offsetof(certv::record, pc) && offsetof(ibft_cert_verdict_t, height) == offsetof(certv::record, height) &&
                    offsetof(ibft_cert_verdict_t, from) == offsetof(certv::record, from) &&
                    offsetof(ibft_cert_verdict_t, pc_hash) == offsetof(certv::record, pc_hash),
                "ABI");
  static_assert(IBFT_CERT_NO_RECORD == certv::NO_RECORD && IBFT_CERT_BIT_SENDER == certv::BIT_SENDER && IBFT_CERT_BIT_HASH == certv::BIT_HASH &&
                    IBFT_CERT_BIT_SELF == certv::BIT_SELF && IBFT_CERT_BIT_HAS_PROPOSAL == certv::BIT_HAS_PROPOSAL &&
                    IBFT_CERT_BIT_HAS_CERTIFICATE == certv::BIT_HAS_CERTIFICATE,
                "ABI");
  static_assert(sizeof(ibft_cert_decision_t) == sizeof(certd::decision) && sizeof(ibft_cert_decision_t) == 64, "ABI");
  static_assert(offsetof(ibft_cert_decision_t, valid_pc) == offsetof(certd::decision, valid_pc) &&
                    offsetof(ibft_cert_decision_t, proposal) == offsetof(certd::decision, proposal) &&
                    offsetof(ibft_cert_decision_t, flags) == offsetof(certd::decision, flags) &&
                    offsetof(ibft_cert_decision_t, prepared_record) == offsetof(certd::decision, prepared_record) &&
                    offsetof(ibft_cert_decision_t, prepared_round) == offsetof(certd::decision, prepared_round) &&
                    offsetof(ibft_cert_decision_t, prepared_hash) == offsetof(certd::decision, prepared_hash) &&
                    offsetof(ibft_cert_decision_t, reserved) == offsetof(certd::decision, reserved),
                "ABI");
  static_assert(IBFT_PROPOSER_ROUNDS_MAX == certd::PROPOSER_ROUNDS_MAX && IBFT_CERT_DECISION_HAS_PREPARED == certd::HAS_PREPARED, "ABI");
  cert_plan p;
  int rc;
  if ((rc = cert_check(c, k, p, /*locked=*/false))) return rc;
  ctx_lock lk(c);
  if ((rc = cert_check(c, k, p, /*locked=*/true))) {
    if (rc != CERT_NOTHING_TO_DO) return rc;
    if (k.round_changes && k.query && k.out_answer) {  // the answer over no records
      rcd::answer none;
      rcd::make_answer(none, rcd::lane_init(), 0u, 0u, 0u);
      memcpy(k.out_answer, &none, sizeof none);
    }
    return IBFT_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  c->wire.columns = false;
  c->staged_n = 0;
  for (auto stage : {cert_reserve, cert_expand, cert_digests, cert_verdicts, cert_compare_and_judge, cert_decide, cert_round_changes, cert_deliver})
    if ((rc = stage(c, k, p))) return rc;
  return IBFT_OK;
}
int ibft_cert_stats(ibft_ctx *c, uint32_t *rows, uint32_t *judged_rows, uint32_t *verdict_rows, uint32_t *unplaced_rows) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (rows) *rows = c->cert.stat[0];
  if (judged_rows) *judged_rows = c->cert.stat[1];
  if (verdict_rows) *verdict_rows = c->cert.stat[2];
  if (unplaced_rows) *unplaced_rows = c->cert.stat[3];
  return IBFT_OK;
}
int ibft_verify_certificates_wire(ibft_ctx *c, const uint8_t *wire_bytes, const uint32_t *off, size_t n, size_t rows_cap,
                                  size_t *out_n_rows, ibft_cert_node_t *out_nodes, ibft_wire_row_t *out_rows,
                                  uint8_t *out_class, uint64_t *out_sender_mask, uint64_t *out_hash_mask,
                                  uint64_t *out_self_mask) {
  cert_call k{};
  k.wire_bytes = wire_bytes, k.off = off, k.n = n, k.rows_cap = rows_cap;
  k.out_n_rows = out_n_rows, k.out_nodes = out_nodes, k.out_rows = out_rows, k.out_class = out_class;
  k.out_sender_mask = out_sender_mask, k.out_hash_mask = out_hash_mask, k.out_self_mask = out_self_mask;
  return certificates_wire_impl(c, k);
}
int ibft_judge_certificates_wire(ibft_ctx *c, const uint8_t *wire_bytes, const uint32_t *off, size_t n, size_t rows_cap, size_t certs_cap,
                                 size_t *out_n_rows, size_t *out_n_certs, ibft_cert_verdict_t *out_cert, ibft_cert_node_t *out_nodes,
                                 ibft_wire_row_t *out_rows, uint8_t *out_class, uint64_t *out_sender_mask, uint64_t *out_hash_mask,
                                 uint64_t *out_self_mask) {
  cert_call k{};
  k.wire_bytes = wire_bytes, k.off = off, k.n = n, k.rows_cap = rows_cap;
  k.judge = true, k.certs_cap = certs_cap, k.out_n_certs = out_n_certs, k.out_cert = out_cert;
  k.out_n_rows = out_n_rows, k.out_nodes = out_nodes, k.out_rows = out_rows, k.out_class = out_class;
  k.out_sender_mask = out_sender_mask, k.out_hash_mask = out_hash_mask, k.out_self_mask = out_self_mask;
  return certificates_wire_impl(c, k);
}

int ibft_decide_certificates_wire(ibft_ctx *c, const uint8_t *wire_bytes, const uint32_t *off, size_t n, size_t rows_cap, size_t certs_cap,
                                  size_t *out_n_rows, size_t *out_n_certs, ibft_cert_verdict_t *out_cert, ibft_cert_decision_t *out_decision,
                                  ibft_cert_node_t *out_nodes, ibft_wire_row_t *out_rows, uint8_t *out_class, uint64_t *out_sender_mask,
                                  uint64_t *out_hash_mask, uint64_t *out_self_mask) {
  cert_call k{};
  k.wire_bytes = wire_bytes, k.off = off, k.n = n, k.rows_cap = rows_cap;
  k.judge = k.decide = true, k.certs_cap = certs_cap, k.out_n_certs = out_n_certs, k.out_cert = out_cert, k.out_decision = out_decision;
  k.out_n_rows = out_n_rows, k.out_nodes = out_nodes, k.out_rows = out_rows, k.out_class = out_class;
  k.out_sender_mask = out_sender_mask, k.out_hash_mask = out_hash_mask, k.out_self_mask = out_self_mask;
  return certificates_wire_impl(c, k);
}

// The decide call plus what handleRoundChangeMessage does with its per-message answers: one quorum record per (height, round)
// of the level-0 ROUND_CHANGE rows and the answer to `query` (round_change_dev.h).  The decide call's checks in its order, the
// new arguments among the argument checks in front.
int ibft_decide_round_changes_wire(ibft_ctx *c, const uint8_t *wire_bytes, const uint32_t *off, size_t n, size_t rows_cap, size_t certs_cap,
                                   size_t *out_n_rows, size_t *out_n_certs, ibft_cert_verdict_t *out_cert, ibft_cert_decision_t *out_decision,
                                   ibft_cert_node_t *out_nodes, ibft_wire_row_t *out_rows, uint8_t *out_class, uint64_t *out_sender_mask,
                                   uint64_t *out_hash_mask, uint64_t *out_self_mask, const ibft_rc_query_t *query, int32_t *out_rc_view,
                                   uint64_t *out_rc_stored, ibft_rc_record_t *out_rc, size_t rc_cap, size_t *out_n_rc, ibft_rc_answer_t *out_answer) {
  static_assert(sizeof(ibft_rc_query_t) == sizeof(rcd::query) && sizeof(ibft_rc_query_t) == 32, "ABI");
  static_assert(sizeof(ibft_rc_record_t) == sizeof(rcd::record) && sizeof(ibft_rc_record_t) == 128, "ABI");
  static_assert(sizeof(ibft_rc_answer_t) == sizeof(rcd::answer) && sizeof(ibft_rc_answer_t) == 64, "ABI");
  static_assert(offsetof(ibft_rc_query_t, min_round) == offsetof(rcd::query, min_round) &&
                    offsetof(ibft_rc_query_t, has_accepted_proposal) == offsetof(rcd::query, has_accepted_proposal) &&
                    offsetof(ibft_rc_record_t, open_rows) == offsetof(rcd::record, open_rows) &&
                    offsetof(ibft_rc_record_t, has_quorum) == offsetof(rcd::record, has_quorum) &&
                    offsetof(ibft_rc_record_t, open_power_lo) == offsetof(rcd::record, open_power_lo) &&
                    offsetof(ibft_rc_record_t, tally) == offsetof(rcd::record, tally) &&
                    offsetof(ibft_rc_answer_t, record) == offsetof(rcd::answer, record) && offsetof(ibft_rc_answer_t, round) == offsetof(rcd::answer, round) &&
                    offsetof(ibft_rc_answer_t, most_round) == offsetof(rcd::answer, most_round) &&
                    offsetof(ibft_rc_answer_t, most_rows) == offsetof(rcd::answer, most_rows) &&
                    offsetof(ibft_rc_answer_t, unjudged_rows) == offsetof(rcd::answer, unjudged_rows),
                "ABI");
  static_assert(IBFT_RC_OVER == rcd::FLAG_OVER && IBFT_RC_VIEW_NONE == rcd::VIEW_NONE && IBFT_RC_VIEW_OVER == rcd::VIEW_OVER, "ABI");
  cert_call k{};
  k.wire_bytes = wire_bytes, k.off = off, k.n = n, k.rows_cap = rows_cap;
  k.judge = k.decide = true, k.certs_cap = certs_cap, k.out_n_certs = out_n_certs, k.out_cert = out_cert, k.out_decision = out_decision;
  k.out_n_rows = out_n_rows, k.out_nodes = out_nodes, k.out_rows = out_rows, k.out_class = out_class;
  k.out_sender_mask = out_sender_mask, k.out_hash_mask = out_hash_mask, k.out_self_mask = out_self_mask;
  k.round_changes = true, k.query = query, k.rc_cap = rc_cap, k.out_rc_view = out_rc_view, k.out_rc_stored = out_rc_stored;
  k.out_rc = out_rc, k.out_n_rc = out_n_rc, k.out_answer = out_answer;
  return certificates_wire_impl(c, k);
}

// The proposer table of the decide call: replaced whole, on the context's stream and waited for (the caller's array is free when
// the call returns; whatever was enqueued before it has run under the table it saw).  A refused call leaves the table alone.
int ibft_set_proposers(ibft_ctx *c, uint64_t height, uint64_t first_round, const uint8_t *proposer20, size_t n_rounds) {
  if (!c || (n_rounds && !proposer20)) return IBFT_E_INVAL;
  if (first_round + (uint64_t)n_rounds < first_round) return IBFT_E_INVAL;  // the range runs past 2^64
  if (n_rounds > IBFT_PROPOSER_ROUNDS_MAX) return IBFT_E_TOOBIG;
  ctx_lock lk(c);
  CertState &s = c->cert;
  if (n_rounds) {
    int rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, s.proposers, (size_t)IBFT_PROPOSER_ROUNDS_MAX * 20))) return rc;
    HIPCHK(c, hipMemcpyAsync(s.proposers.p, proposer20, n_rounds * 20, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  s.prop_height = n_rounds ? height : 0;
  s.prop_first = n_rounds ? first_round : 0;
  s.prop_rounds = (uint32_t)n_rounds;
  return IBFT_OK;
}
int ibft_proposers_info(ibft_ctx *c, uint64_t *height, uint64_t *first_round, uint32_t *n_rounds) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (height) *height = c->cert.prop_height;
  if (first_round) *first_round = c->cert.prop_first;
  if (n_rounds) *n_rounds = c->cert.prop_rounds;
  return IBFT_OK;
}

int ibft_wire_stage_seals(ibft_ctx *c) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (!c->wire.columns) return IBFT_E_INVAL;  // no parsed batch resident (another call restaged the columns)
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t n = c->wire.rows;
  if (n) {
    hipLaunchKernelGGL(ibftk::wire_stage_seals_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream,
                       (const wire::row_info *)c->d_wire_rows.p, (const uint8_t *)c->d_seal.p, n,
                       (uint8_t *)c->d_hash.p, (uint8_t *)c->d_sig.p, (uint8_t *)c->d_pre.p);
    HIPCHK(c, hipGetLastError());
    int rc = apply_seal_digest(c, c->d_hash.p, n);
    if (rc) return rc;
  }
  c->staged_pre = true;
  return IBFT_OK;
}

static int tally_impl(ibft_ctx *c, const uint8_t *sender20, const uint64_t *mask, size_t n, const uint8_t *proposer20,
                      ibft_tally_t *tally);
int ibft_tally(ibft_ctx *c, const uint8_t *sender20, const uint64_t *mask, size_t n, ibft_tally_t *tally) {
  return tally_impl(c, sender20, mask, n, nullptr, tally);
}
int ibft_tally_prepare(ibft_ctx *c, const uint8_t *sender20, const uint64_t *mask, size_t n, const uint8_t proposer20[20],
                       ibft_tally_t *tally) {
  if (!proposer20) return IBFT_E_INVAL;
  return tally_impl(c, sender20, mask, n, proposer20, tally);
}
static int tally_impl(ibft_ctx *c, const uint8_t *sender20, const uint64_t *mask, size_t n, const uint8_t *proposer20,
                      ibft_tally_t *tally) {
  if (!c || !tally || (n && (!sender20 || !mask))) return IBFT_E_INVAL;
  ctx_lock lk(c);
  if (n > c->max_rows) return IBFT_E_TOOBIG;
  if (!c->have_valset) return IBFT_E_NOVALSET;
  HIPCHK(c, hipSetDevice(c->device));
  // resolve sender -> validator index with a small lookup pass over the table in HBM
  int rc;
  c->wire.columns = false;
  if ((rc = upload(c, c->d_signer, sender20, n * 20))) return rc;
  c->mask_dirty_words = std::max(c->mask_dirty_words, (uint32_t)mask_words(n));
  if ((rc = upload(c, c->d_mask, mask, (size_t)mask_words(n) * 8))) return rc;
  ibftk::lookup_proposer lp{};
  if (proposer20) {
    lp.on = 1;
    memcpy(lp.a, proposer20, 20);
  }
  if (n) {
    hipLaunchKernelGGL(ibftk::lookup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       (const uint8_t *)c->d_signer.p, (const uint32_t *)c->d_vtab.p, c->vslot_mask,
                       (uint32_t)n, (int32_t *)c->d_vidx.p, lp);
    HIPCHK(c, hipGetLastError());
  }
  note_proposer(c, proposer20);
  if ((rc = enqueue_tally(c, (uint32_t)n))) return rc;
  return fetch_results(c, (uint32_t)n, nullptr, tally, true);
}


/* ---- multi-GPU: validator shards + one RCCL all-reduce of verdict words and tally partials ---- */
int ibft_shard_range(uint64_t n_total, uint32_t rank, uint32_t world, uint64_t *lo, uint64_t *hi) {
  if (!world || rank >= world || !lo || !hi) return IBFT_E_INVAL;
  const uint64_t per = shard_rows_per_rank(n_total, world);
  *lo = std::min<uint64_t>((uint64_t)rank * per, n_total);
  *hi = std::min<uint64_t>(*lo + per, n_total);
  return IBFT_OK;
}

int ibft_exchange_layout(uint64_t n_total, uint32_t world, uint32_t n_validators, uint32_t n_masks, uint32_t *words_per_rank,
                         uint32_t *seen_words, uint32_t *slots) {
  if (!world || (n_masks != 1 && n_masks != 2)) return IBFT_E_INVAL;
  const uint64_t w = shard_rows_per_rank(n_total, world) / 64;
  if (words_per_rank) *words_per_rank = (uint32_t)w;
  if (seen_words) *seen_words = (n_validators + 63) / 64;
  if (slots) *slots = exchange_slots(n_masks, (uint32_t)w, world, n_validators);
  return IBFT_OK;
}

int ibft_comm_preload(void) { return rccl() ? IBFT_OK : IBFT_E_RCCL; }

int ibft_comm_unique_id(uint8_t id[IBFT_COMM_ID_BYTES]) {
  static_assert(IBFT_COMM_ID_BYTES == sizeof(ncclUniqueId), "ABI");
  if (!id) return IBFT_E_INVAL;
  RcclApi *api = rccl();
  if (!api) return IBFT_E_RCCL;
  ncclUniqueId u;
  if (api->GetUniqueId(&u) != ncclSuccess) return IBFT_E_RCCL;
  memcpy(id, &u, sizeof u);
  return IBFT_OK;
}

int ibft_comm_init(ibft_ctx *c, const uint8_t id[IBFT_COMM_ID_BYTES], uint32_t rank, uint32_t world) {
  if (!c || !id || !world || rank >= world) return IBFT_E_INVAL;
  RcclApi *api = rccl();
  if (!api) return IBFT_E_RCCL;
  ctx_lock lk(c);
  if (c->comm) return IBFT_E_INVAL;
  HIPCHK(c, hipSetDevice(c->device));
  ncclUniqueId u;
  memcpy(&u, id, sizeof u);
  ncclComm_t comm = nullptr;
  NCCLCHK(c, api, api->CommInitRank(&comm, (int)world, u, (int)rank));  // collective: blocks until every rank has joined
  return comm_attach(c, comm, rank, world);
}

int ibft_comm_destroy(ibft_ctx *c) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  (void)hipSetDevice(c->device);
  if (c->xstream) (void)hipStreamSynchronize(c->xstream);
  comm_release(c);
  return IBFT_OK;
}

int ibft_seals_exchange(ibft_ctx *c, uint64_t n_total) {
  if (!c) return IBFT_E_INVAL;
  if (c->xlocal) return IBFT_E_INVAL;  // a rank of a local group: only the group can run the collective
  RcclApi *api = rccl();
  if (!api) return IBFT_E_RCCL;
  ctx_lock lk(c);
  xplan x{};
  int rc;
  if ((rc = exchange_pre(c, n_total, x))) return rc;
  if ((rc = exchange_collective(c, api, x))) return rc;
  return exchange_post(c, n_total, x);
}

int ibft_comm_info(ibft_ctx *c, uint32_t *rccl_nranks, uint32_t *rccl_rank, int32_t *rccl_device) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  RcclApi *api = rccl();
  if (!c->comm || !api || !api->CommCount || !api->CommUserRank || !api->CommCuDevice) return IBFT_E_INVAL;
  int n = 0, r = 0, d = 0;
  NCCLCHK(c, api, api->CommCount(c->comm, &n));
  NCCLCHK(c, api, api->CommUserRank(c->comm, &r));
  NCCLCHK(c, api, api->CommCuDevice(c->comm, &d));
  if (rccl_nranks) *rccl_nranks = (uint32_t)n;
  if (rccl_rank) *rccl_rank = (uint32_t)r;
  if (rccl_device) *rccl_device = d;
  return IBFT_OK;
}

int ibft_seals_fetch_merged(ibft_ctx *c, uint64_t *out_mask, ibft_tally_t *tally) {
  if (!c) return IBFT_E_INVAL;
  ctx_lock lk(c);
  return fetch_merged_locked(c, out_mask, tally);
}

int ibft_group_create(const int32_t *devices, uint32_t n_dev, uint32_t flags, uint32_t max_rows_total, ibft_group **out) {
  if (!out || !devices || !n_dev || n_dev > (uint32_t)ibftk::XSUM_MAX_RANKS) return IBFT_E_INVAL;
  *out = nullptr;
  // Which collective: RCCL needs one rank per DEVICE.  A group that lists a device more than once (several contexts
  // sharing one MI355X: how the exchange is exercised with W > 1 on a one-GPU box) — or IBFT_GROUP_COLLECTIVE=local
  // with peer-accessible devices — sums the buffers with the library's own kernel instead.
  bool local = false;
  for (uint32_t i = 0; i < n_dev; i++)
    for (uint32_t j = 0; j < i; j++) local = local || devices[i] == devices[j];
  const char *mode = getenv("IBFT_GROUP_COLLECTIVE");
  if (mode && !strcmp(mode, "local")) local = true;
  RcclApi *api = local ? nullptr : rccl();
  if (!local && !api) return IBFT_E_RCCL;
  ibft_group *g = new (std::nothrow) ibft_group();
  if (!g) return IBFT_E_NOMEM;
  g->local = local;
  const uint64_t total = max_rows_total ? max_rows_total : (uint64_t)DEFAULT_MAX_ROWS * n_dev;
  int rc = IBFT_OK;
  for (uint32_t i = 0; i < n_dev && rc == IBFT_OK; i++) {
    ibft_cfg cfg{devices[i], flags, (uint32_t)shard_rows_per_rank(total, n_dev), IBFT_KERNEL_AUTO};
    ibft_ctx *c = nullptr;
    rc = ibft_ctx_create(&cfg, &c);
    if (rc == IBFT_OK) g->ctx.push_back(c);
  }
  if (rc == IBFT_OK && local) {
    // rank 0's device must be able to address every rank's exchange buffer
    for (uint32_t i = 1; i < n_dev && rc == IBFT_OK; i++) {
      if (devices[i] == devices[0]) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, devices[0], devices[i]) != hipSuccess || !can) {
        rc = IBFT_E_INVAL;
        break;
      }
      (void)hipSetDevice(devices[0]);
      const hipError_t e = hipDeviceEnablePeerAccess(devices[i], 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) rc = IBFT_E_HIP;
      (void)hipGetLastError();
    }
    for (uint32_t i = 0; i < n_dev && rc == IBFT_OK; i++) rc = comm_attach(g->ctx[i], nullptr, i, n_dev);
  } else if (rc == IBFT_OK) {
    ncclUniqueId u;
    std::vector<ncclComm_t> comms(n_dev, nullptr);
    // one thread initialises every rank: the calls only complete inside the group (ncclCommInitRank's contract)
    bool ok = api->GetUniqueId(&u) == ncclSuccess && api->GroupStart() == ncclSuccess;
    for (uint32_t i = 0; ok && i < n_dev; i++)
      ok = hipSetDevice(devices[i]) == hipSuccess && api->CommInitRank(&comms[i], (int)n_dev, u, (int)i) == ncclSuccess;
    ok = api->GroupEnd() == ncclSuccess && ok;
    for (uint32_t i = 0; ok && i < n_dev; i++) ok = comm_attach(g->ctx[i], comms[i], i, n_dev) == IBFT_OK;
    if (!ok) rc = IBFT_E_RCCL;
  }
  if (rc != IBFT_OK) {
    ibft_group_destroy(g);
    return rc;
  }
  if (n_dev > 1)
    for (uint32_t i = 0; i < n_dev; i++) g->worker.emplace_back(new GroupWorker());
  *out = g;
  return IBFT_OK;
}

void ibft_group_destroy(ibft_group *g) {
  if (!g) return;
  g->worker.clear();  // joins the threads
  for (ibft_ctx *c : g->ctx) ibft_ctx_destroy(c);
  delete g;
}
int ibft_group_is_local(const ibft_group *g) { return g ? (g->local ? 1 : 0) : IBFT_E_INVAL; }

uint32_t ibft_group_size(const ibft_group *g) { return g ? (uint32_t)g->ctx.size() : 0; }
ibft_ctx *ibft_group_ctx(ibft_group *g, uint32_t i) { return (g && i < g->ctx.size()) ? g->ctx[i] : nullptr; }

int ibft_set_seal_digest(ibft_ctx *c, uint32_t mode, const uint8_t *suffix, size_t suffix_len) {
  if (!c || mode > IBFT_SEAL_DIGEST_KECCAK_SUFFIX || (suffix_len && !suffix) || suffix_len > IBFT_SEAL_SUFFIX_MAX) return IBFT_E_INVAL;
  ctx_lock lk(c);
  uint8_t block[72] = {0};
  if (mode == IBFT_SEAL_DIGEST_KECCAK_SUFFIX) {
    if (suffix_len) memcpy(block, suffix, suffix_len);
    block[suffix_len] = 0x01;  // pad10*1 starts right behind the message
  }
  c->seal_digest_mode = mode;
  memcpy(c->seal_suffix_words, block, sizeof block);
  c->staged_n = 0;  // a resident batch was staged under the previous convention
  c->wire.columns = false;
  return IBFT_OK;
}
int ibft_group_set_seal_digest(ibft_group *g, uint32_t mode, const uint8_t *suffix, size_t suffix_len) {
  if (!g) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  for (ibft_ctx *c : g->ctx) {
    int rc = ibft_set_seal_digest(c, mode, suffix, suffix_len);
    if (rc) return rc;
  }
  return IBFT_OK;
}

int ibft_group_set_validators(ibft_group *g, uint64_t height, const uint8_t *addrs20, const uint64_t *power, size_t n) {
  if (!g) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  // the validator table is replicated on every device (28 B per validator); every device on its own thread
  return g->each([&](uint32_t i) { return ibft_set_validators(g->ctx[i], height, addrs20, power, n); });
}

int ibft_group_set_validators_u256(ibft_group *g, uint64_t height, const uint8_t *addrs20, const uint8_t *power_be32, size_t n) {
  if (!g) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  return g->each([&](uint32_t i) { return ibft_set_validators_u256(g->ctx[i], height, addrs20, power_be32, n); });
}

// the exchange of a group call: every rank packed (exchange_pre) → collective → unpack → results of rank 0 to the caller
static int group_exchange(ibft_group *g, uint64_t n, std::vector<xplan> &plan, uint64_t *out_mask, uint64_t *out_mask2,
                          ibft_tally_t *tally) {
  const uint32_t world = (uint32_t)g->ctx.size();
  int rc;
  if (g->local) {
    if ((rc = exchange_collective_local(g->ctx, plan))) return rc;
  } else {
    RcclApi *api = rccl();
    if (!api) return IBFT_E_RCCL;
    // single thread: the calls go inside a group
    bool ok = api->GroupStart() == ncclSuccess;
    for (uint32_t i = 0; ok && i < world; i++) ok = exchange_collective(g->ctx[i], api, plan[i]) == IBFT_OK;
    ok = api->GroupEnd() == ncclSuccess && ok;
    if (!ok) return IBFT_E_RCCL;
  }
  for (uint32_t i = 0; i < world; i++)
    if ((rc = exchange_post(g->ctx[i], n, plan[i]))) return rc;
  for (uint32_t i = world; i-- > 0;)  // every rank holds the merged result; device 0's copy is handed to the caller
    if ((rc = fetch_merged_locked(g->ctx[i], i == 0 ? out_mask : nullptr, i == 0 ? tally : nullptr, i == 0 ? out_mask2 : nullptr)))
      return rc;
  return IBFT_OK;
}

int ibft_group_verify_seals(ibft_group *g, const uint8_t *hash32, const uint8_t *sig65, const uint8_t *signer20,
                            const uint8_t *pre_flags, size_t n, uint64_t *out_mask, ibft_tally_t *tally) {
  if (!g || (n && (!hash32 || !sig65 || !signer20 || !out_mask))) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  const uint32_t world = (uint32_t)g->ctx.size();
  std::vector<std::unique_lock<std::mutex>> locks;
  for (ibft_ctx *c : g->ctx) locks.emplace_back(c->mu);
  for (ibft_ctx *c : g->ctx)
    if (!c->have_valset) return IBFT_E_NOVALSET;
  // every device verifies its own 64-aligned row range: stage, verdict kernel, tally, pack — all asynchronous past the
  // upload, every device driven by its own host thread
  std::vector<xplan> plan(world);
  int rc = g->each([&](uint32_t i) {
    ibft_ctx *c = g->ctx[i];
    uint64_t lo, hi;
    (void)ibft_shard_range(n, i, world, &lo, &hi);
    int r;
    if ((r = seals_stage_locked(c, hash32 + 32 * lo, sig65 + 65 * lo, signer20 + 20 * lo, pre_flags ? pre_flags + lo : nullptr,
                                (size_t)(hi - lo), false)))
      return r;
    if ((r = seals_launch_locked(c, 1))) return r;
    return exchange_pre(c, n, plan[i], 1);
  });
  if (rc) return rc;
  return group_exchange(g, n, plan, out_mask, nullptr, tally);
}

// rows [lo, hi) of a payload column as a column of their own: offsets rebased to the shard's first byte
static void shard_offsets(const uint32_t *off, uint64_t lo, uint64_t hi, std::vector<uint32_t> &out) {
  out.resize((size_t)(hi - lo) + 1);
  for (uint64_t i = lo; i <= hi; i++) out[(size_t)(i - lo)] = off[i] - off[lo];
}

int ibft_group_verify_senders(ibft_group *g, const uint8_t *payload, const uint32_t *off, const uint8_t *sig65,
                              const uint8_t *from20, const uint8_t *pre_flags, size_t n, uint64_t *out_mask,
                              ibft_tally_t *tally) {
  if (!g || (n && (!off || !sig65 || !from20 || !out_mask))) return IBFT_E_INVAL;
  if (!offsets_ok(off, n)) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  const uint32_t world = (uint32_t)g->ctx.size();
  std::vector<std::unique_lock<std::mutex>> locks;
  for (ibft_ctx *c : g->ctx) locks.emplace_back(c->mu);
  std::vector<xplan> plan(world);
  std::vector<std::vector<uint32_t>> loff(world);
  int rc = g->each([&](uint32_t i) {
    ibft_ctx *c = g->ctx[i];
    uint64_t lo, hi;
    (void)ibft_shard_range(n, i, world, &lo, &hi);
    if (n) shard_offsets(off, lo, hi, loff[i]);
    int r = senders_launch_locked(c, n ? payload + off[lo] : nullptr, n ? loff[i].data() : nullptr, sig65 + 65 * lo,
                                  from20 + 20 * lo, pre_flags ? pre_flags + lo : nullptr, (size_t)(hi - lo));
    if (r) return r;
    return exchange_pre(c, n, plan[i], 1);
  });
  if (rc) return rc;
  return group_exchange(g, n, plan, out_mask, nullptr, tally);
}

int ibft_group_verify_messages(ibft_group *g, const uint8_t *payload, const uint32_t *off, const uint8_t *msg_sig65,
                               const uint8_t *from20, const uint8_t *hash32, const uint8_t *hash_len, const uint8_t *seal65,
                               const uint8_t *sender_pre, const uint8_t *valid_pre, size_t n, const uint8_t *raw,
                               size_t raw_len, uint64_t round, const uint8_t *digest32, const uint8_t *proposer20,
                               uint64_t *out_sender_mask, uint64_t *out_valid_mask, ibft_tally_t *tally) {
  if (!g || (n && (!off || !msg_sig65 || !from20 || !hash32 || !hash_len || !out_sender_mask || !out_valid_mask)))
    return IBFT_E_INVAL;
  if (!offsets_ok(off, n)) return IBFT_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  const uint32_t world = (uint32_t)g->ctx.size();
  std::vector<std::unique_lock<std::mutex>> locks;
  for (ibft_ctx *c : g->ctx) locks.emplace_back(c->mu);
  std::vector<xplan> plan(world);
  std::vector<std::vector<uint32_t>> loff(world);
  // every device judges its own 64-aligned range of MESSAGES completely (both signatures of a COMMIT are rows of its
  // one verdict launch); the proposal is hashed (and remembered) by every device for itself
  int rc = g->each([&](uint32_t i) {
    ibft_ctx *c = g->ctx[i];
    uint64_t lo, hi;
    (void)ibft_shard_range(n, i, world, &lo, &hi);
    if (n) shard_offsets(off, lo, hi, loff[i]);
    note_proposer(c, proposer20, /*shard=*/true);
    int r = messages_launch_locked(c, n ? payload + off[lo] : nullptr, n ? loff[i].data() : nullptr, msg_sig65 + 65 * lo,
                                   from20 + 20 * lo, hash32 + 32 * lo, hash_len + lo, seal65 ? seal65 + 65 * lo : nullptr,
                                   sender_pre ? sender_pre + lo : nullptr, valid_pre ? valid_pre + lo : nullptr,
                                   (size_t)(hi - lo), raw, raw_len, round, digest32);
    c->next_prop_on = c->next_shard = false;
    if (r) return r;
    return exchange_pre(c, n, plan[i], 2, proposer20);
  });
  if (rc) {
    for (ibft_ctx *c : g->ctx) c->have_H = false;
    return rc;
  }
  return group_exchange(g, n, plan, out_sender_mask, out_valid_mask, tally);
}

// Certificates sharded by CARRIER: every device expands and judges the trees of its own contiguous range of the call's
// messages (ibft_verify_certificates_wire on its context, all devices at once); nothing has to be exchanged — the verdicts
// are per row and no tally is taken — so the only work here is the renumbering: the merged rows are in the breadth-first
// order ONE call over all n messages would produce (level by level, within a level rank by rank, which is message order).
int ibft_group_verify_certificates_wire(ibft_group *g, const uint8_t *wire_bytes, const uint32_t *off, size_t n, size_t rows_cap,
                                        size_t *out_n_rows, ibft_cert_node_t *out_nodes, ibft_wire_row_t *out_rows,
                                        uint8_t *out_class, uint64_t *out_sender_mask, uint64_t *out_hash_mask,
                                        uint64_t *out_self_mask) {
  if (!g || !out_n_rows || (n && (!off || !out_sender_mask))) return IBFT_E_INVAL;
  if (!offsets_ok(off, n)) return IBFT_E_INVAL;
  *out_n_rows = 0;
  if (n == 0) return IBFT_OK;
  std::lock_guard<std::mutex> lk(g->mu);
  const uint32_t world = (uint32_t)g->ctx.size();
  const size_t per = (n + world - 1) / world;
  struct Part {
    size_t lo = 0, hi = 0, rows = 0;
    uint32_t shift = 0;  // bytes in front of the shard's first message in the buffer its device sees
    std::vector<uint32_t> off;
    std::vector<ibft_cert_node_t> nodes;
    std::vector<ibft_wire_row_t> wrows;
    std::vector<uint8_t> cls;
    std::vector<uint64_t> ms, mh, mself;
  };
  std::vector<Part> part(world);
  int rc = g->each([&](uint32_t i) {
    Part &p = part[i];
    p.lo = std::min(n, (size_t)i * per);
    p.hi = std::min(n, p.lo + per);
    if (p.hi == p.lo) return (int)IBFT_OK;
    ibft_ctx *c = g->ctx[i];
    const size_t cap = std::min<size_t>(rows_cap, c->max_rows), words = (cap + 63) / 64;
    // (a shard that does not start the buffer keeps a few bytes in front of it: no message of it lies at offset 0, so a
    // node's raw_off of 0 can only mean "not parsed" and the offsets can be moved back into the whole buffer below)
    p.shift = std::min<uint32_t>(off[p.lo], 64u);
    p.off.resize(p.hi - p.lo + 1);
    for (size_t k = p.lo; k <= p.hi; k++) p.off[k - p.lo] = off[k] - off[p.lo] + p.shift;
    p.nodes.resize(cap);
    if (out_rows) p.wrows.resize(cap);
    p.cls.assign(cap, 0);
    p.ms.assign(words, 0);
    p.mh.assign(words, 0);
    p.mself.assign(words, 0);
    return ibft_verify_certificates_wire(c, wire_bytes + off[p.lo] - p.shift, p.off.data(), p.hi - p.lo, cap, &p.rows, p.nodes.data(),
                                         out_rows ? p.wrows.data() : nullptr, p.cls.data(), p.ms.data(), p.mh.data(), p.mself.data());
  });
  if (rc) return rc;
  // rows per (rank, level); a rank's rows are breadth first, so its levels are contiguous blocks
  size_t total = 0, levels = 1;
  for (Part &p : part) {
    total += p.rows;
    for (size_t j = 0; j < p.rows; j++) levels = std::max<size_t>(levels, (size_t)p.nodes[j].level + 1);
  }
  if (total > rows_cap) return IBFT_E_TOOBIG;
  std::vector<std::vector<size_t>> count(world, std::vector<size_t>(levels + 2, 0)), start(world, std::vector<size_t>(levels + 2, 0)),
      dest(world, std::vector<size_t>(levels + 2, 0));
  for (uint32_t r = 0; r < world; r++) {
    for (size_t j = 0; j < part[r].rows; j++) count[r][part[r].nodes[j].level]++;
    for (size_t l = 1; l < levels + 2; l++) start[r][l] = start[r][l - 1] + count[r][l - 1];
  }
  size_t base = 0;
  for (size_t l = 0; l < levels + 2; l++)
    for (uint32_t r = 0; r < world; r++) {
      dest[r][l] = base;
      base += count[r][l];
    }
  const size_t words = (total + 63) / 64;
  memset(out_sender_mask, 0, words * 8);
  if (out_hash_mask) memset(out_hash_mask, 0, words * 8);
  if (out_self_mask) memset(out_self_mask, 0, words * 8);
  for (uint32_t r = 0; r < world; r++) {
    const Part &p = part[r];
    const uint32_t byte_base = p.rows ? off[p.lo] - p.shift : 0;
    auto global = [&](size_t local, size_t level) { return dest[r][level] + (local - start[r][level]); };
    for (size_t j = 0; j < p.rows; j++) {
      const size_t level = p.nodes[j].level, at = global(j, level);
      if (out_nodes) {
        ibft_cert_node_t nd = p.nodes[j];
        nd.off += byte_base;
        if (nd.raw_off) nd.raw_off += byte_base;
        if (nd.parent == IBFT_CERT_NO_PARENT)
          nd.ordinal += (uint32_t)p.lo;  // its number among the call's messages
        else
          nd.parent = (uint32_t)global(nd.parent, level - 1);
        // a leaf's first_child is whatever the walk left there: only a node WITH children has a range to renumber (round-3
        // advice: the subtraction underflowed for leaves and consumers that test the bounds first took the slow route)
        nd.first_child = nd.n_children ? (uint32_t)global(nd.first_child, level + 1) : (uint32_t)at;
        out_nodes[at] = nd;
      }
      if (out_rows) out_rows[at] = p.wrows[j];
      if (out_class) out_class[at] = p.cls[j];
      const uint64_t bit = 1ull << (at & 63);
      if ((p.ms[j >> 6] >> (j & 63)) & 1) out_sender_mask[at >> 6] |= bit;
      if (out_hash_mask && ((p.mh[j >> 6] >> (j & 63)) & 1)) out_hash_mask[at >> 6] |= bit;
      if (out_self_mask && ((p.mself[j >> 6] >> (j & 63)) & 1)) out_self_mask[at >> 6] |= bit;
    }
  }
  *out_n_rows = total;
  return IBFT_OK;
}

}  // extern "C"
