/*
 * include/ibftgpu.h — C ABI of libibftgpu.so, the MI355X (gfx950) batch verifier
 * that sits behind go-ibft's Verifier hooks.
 *
 * This is the drop-in boundary: plain pointers and sizes, no
 * framework types.  The Go side keeps core/ibft.go's RunSequence untouched and
 * calls these entry points through the cgo shim in shim/go/ (see INTEGRATION.md).
 *
 * Each entry point replaces a per-message interface call of the reference with one
 * call per batch:
 *
 *   ibft_verify_hashes   <- Verifier.IsValidProposalHash(proposal, hash)
 *                           /root/reference/core/backend.go:50-51; call sites
 *                           /root/reference/core/ibft.go:545, 649, 781, 858, 938
 *   ibft_verify_seals    <- Verifier.IsValidCommittedSeal(proposalHash, seal)
 *                           /root/reference/core/backend.go:53-55; call site
 *                           /root/reference/core/ibft.go:943
 *   ibft_recover_seals, ibft_recover_block_seals
 *                        <- the same for BARE committed seals (finalized headers that carry only signatures): the signer
 *                           is what ecrecover returns — address out, membership of the recovered address, HasQuorum
 *   ibft_proposal_hashes, ibft_verify_block_seals_raw, ibft_recover_block_seals_raw
 *                        <- chain sync from (Proposal, []CommittedSeal) pairs (core/backend.go:80-82): the proposal hash of
 *                           every block — keccak256(RawProposal ‖ BE64(Round)), what IsValidProposalHash recomputes
 *                           (core/backend.go:50-51) — on the device, alone or in front of the two block calls above
 *   ibft_verify_senders  <- Verifier.IsValidValidator(msg)
 *                           /root/reference/core/backend.go:41-45; call sites
 *                           /root/reference/core/ibft.go:735, 1128, 1213, 1220
 *   ibft_set_validators  <- ValidatorBackend.GetVotingPowers(height)
 *                           /root/reference/core/validator_manager.go:17-20, 50-75
 *   ibft_tally (+ the ibft_tally_t filled by the verify calls)
 *                        <- ValidatorManager.HasQuorum
 *                           /root/reference/core/validator_manager.go:77-96
 *   ibft_tally_prepare (+ the proposer20 argument of the message-set calls)
 *                        <- ValidatorManager.HasPrepareQuorum — the decision hasQuorumByMsgType takes for PREPARE
 *                           /root/reference/core/validator_manager.go:99-127, core/ibft.go:1273-1284
 *   ibft_verify_messages, ibft_verify_messages_wire
 *                        <- all of the above for a whole PREPARE / COMMIT set in ONE call (from SoA columns / from the
 *                           transport's bytes): IsValidValidator on arrival (core/ibft.go:1128) and the closure of
 *                           handlePrepare / handleCommit (:856-862, :932-944) are pure, so a message is judged once,
 *                           completely — both signatures of a COMMIT in one verdict launch
 *   ibft_verify_senders_wire, ibft_wire_stage_seals
 *                        <- proto.Unmarshal + PayloadNoSig (messages/proto/helper.go:12-27) + IsValidValidator
 *   ibft_verify_certificates_wire
 *                        <- every IsValidValidator / IsValidProposalHash that validateProposal, validPC and
 *                           handleRoundChangeMessage ask about the messages NESTED in PREPREPARE / ROUND_CHANGE
 *                           messages (core/ibft.go:470-551, 683-788), from the transport's bytes
 *   ibft_judge_certificates_wire
 *                        <- the same, and validPC / AreValidPCMessages / HasUniqueSenders (core/ibft.go:1162-1231,
 *                           messages/helpers.go:148-213) and the RoundChangeCertificate half of validateProposal
 *                           (core/ibft.go:697-778) themselves, per certificate, up to IsProposer: one record per carrier
 *   ibft_set_proposers, ibft_decide_certificates_wire
 *                        <- Backend.IsProposer (core/backend.go:47-48) as a table of one height, and with it validPC whole,
 *                           handleRoundChangeMessage's closure and validateProposal with its closing
 *                           IsValidProposalHash (core/ibft.go:478-489, 640-787): one decision per record
 *   ibft_comm_*, ibft_group_*  validator shards over several MI355X, one RCCL all-reduce inside the library
 *   ibft_sign_seals, ibft_sign_seals_ex
 *                        <- n × Backend.BuildCommitMessage's seal (core/backend.go:12-34), simulators only (_ex: with
 *                           RFC 6979 nonces, the seals third-party signers reproduce)
 *   ibft_sign_messages_wire
 *                        <- n × Backend.BuildPrepareMessage / BuildCommitMessage (core/backend.go:12-34) as wire bytes,
 *                           simulators only: what ibft_verify_senders_wire / ibft_verify_messages_wire read
 *   ibft_sign_envelopes_wire
 *                        <- n × Backend.BuildPrePrepareMessage / BuildRoundChangeMessage around given bodies, simulators
 *                           only: what ibft_verify_certificates_wire reads
 *   ibft_pinned_alloc    page-locked column buffers the device reads itself (one gather launch per call)
 *
 * Conventions (the reference fixes none of the arithmetic; these are the
 * Ethereum-style ones an IBFT backend uses, stated once, obeyed by CPU oracle and
 * GPU alike):
 *   proposal hash = keccak256(RawProposal ‖ BE64(Round));  seal digest = the 32-byte
 *   proposalHash itself (or keccak256(proposalHash ‖ suffix): ibft_set_seal_digest);  sender digest = keccak256(PayloadNoSig)
 *   (/root/reference/messages/proto/helper.go:12-27);  signature = 65 B r‖s‖v with
 *   r,s big-endian in [1,n-1] and v∈{0,1};  address = keccak256(X‖Y)[12:32].
 *   Recovery-id policy: v is the parity of R.y and nothing else — R.x = r always.  The second candidate
 *   of SEC 1 §4.1.6 (R.x = r + n, possible only for r < p − n ≈ 2^128.4, i.e. with probability ≈ 2^−127.6,
 *   recovery ids 2 and 3) is NEVER tried: v ∈ {2,3} (and every other value) is rejected by every kernel
 *   variant, cold and warm, exactly as go-ethereum's crypto.Ecrecover / the precompile reject it for a
 *   65-byte [R‖S‖V] input with V > 1.  High-s signatures are accepted unless IBFT_FLAG_STRICT_LOW_S.
 *
 * Verdict masks: bit i of out_mask[i/64] is row i's verdict (1 = the reference
 * predicate would return true).  Rows the host already knows to be structurally
 * invalid (nil payload, wrong length, a1 failed → a2 short-circuited,
 * /root/reference/core/ibft.go:938-943) are passed with a non-zero pre_flags byte
 * and come back 0 without touching the device arithmetic.
 *
 * Error behaviour: every call returns IBFT_OK (0) or a negative IBFT_E_* code and
 * never synthesises verdicts on failure — the caller must then run its own CPU
 * Verifier for that batch (all-false would stall liveness, all-true would break
 * safety).  There is NO CPU fallback inside this library.
 *
 * Threading: a context is internally serialised (one mutex, one HIP stream + a side stream for the proposal hash); use
 * one context per concurrent caller (the four goroutines of
 * /root/reference/core/ibft.go:335-347 would each hold one).  Nothing is retained
 * from caller memory after a call returns (cgo pointer rules).
 */
#ifndef IBFTGPU_H
#define IBFTGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBFT_OK 0
#define IBFT_E_INVAL (-1)     /* bad argument                                   */
#define IBFT_E_NODEVICE (-2)  /* no usable gfx950 device / HIP runtime error     */
#define IBFT_E_NOMEM (-3)     /* host or device allocation failed                */
#define IBFT_E_HIP (-4)       /* a HIP call failed; ibft_last_error() has detail */
#define IBFT_E_NOVALSET (-5)  /* ibft_set_validators has not succeeded yet       */
#define IBFT_E_POWER (-6)     /* total voting power is zero (errVotingPowerNotCorrect) */
#define IBFT_E_TOOBIG (-7)    /* batch larger than cfg.max_rows                  */
#define IBFT_E_RCCL (-8)      /* librccl could not be loaded, or a collective / communicator call failed */

/* cfg.flags */
#define IBFT_FLAG_STRICT_LOW_S 1u /* also reject s > n/2 (off: go-ethereum Ecrecover semantics) */
/* Warm path: remember each validator's public key the first time it is recovered (and hashes to
 * its address), build per-validator fixed-base tables in HBM (655 KB per validator, budget
 * IBFT_QTAB_BUDGET_GB, default 64) and VERIFY later signatures of that validator against them
 * instead of recovering — identical verdicts (csrc/verify_dev.h), ~4-10x less work.  The tables are
 * per DEVICE and per ADDRESS (ibft_cache_memory below): shared by every context of the device, kept
 * for every validator that stays in the set when ibft_set_validators changes it.                */
#define IBFT_FLAG_PUBKEY_CACHE 2u
/* Certificate calls (ibft_verify_certificates_wire, ibft_judge_certificates_wire) judge each distinct (digest, signature,
 * From) once — see "certificates: identical nested messages" below.  Off by default; the environment variable
 * IBFT_CERT_DEDUP=0|1, read at ibft_ctx_create, overrides the flag either way.  Leaving it on where nothing repeats costs
 * the table, the compaction and one more synchronisation: +0.05 ms per call at 4 224 distinct rows on a cold context,
 * nothing measurable with known keys; where almost everything repeats (a round change at N = 1 024, 467 172 rows) the
 * call takes 6.7 instead of 11.3 ms cold, 6.5 instead of 8.2 ms with known keys.                   */
#define IBFT_FLAG_CERT_DEDUP 4u
/* The flat wire calls (ibft_verify_senders_wire, ibft_verify_messages_wire) also judge PREPARE / COMMIT messages in a
 * non-canonical encoding — fields out of order, padded varints, explicit defaults, repeated fields — instead of marking
 * them IBFT_WIRE_NEEDS_HOST: see "the recode class" at ibft_verify_senders_wire.  Off by default; the environment variable
 * IBFT_WIRE_RECODE=0|1, read at ibft_ctx_create, overrides the flag either way.  Off: no extra launch, every output bit
 * for bit as before.  On: one more small launch per call; a batch of canonical rows gives bit for bit the flag-off
 * outputs.  N = 4 096 COMMIT messages, known keys: a canonical batch 0.300 ms off, 0.304 ms on (two
 * flag-off legs of the same loop differ by 0.001); every row in another encoding 0.41 ms, against 1.67 ms through host
 * decode and re-marshal.  The certificate calls ignore the flag; there is no streamed form.                                      */
#define IBFT_FLAG_WIRE_RECODE 8u

/* pre_flags bits */
#define IBFT_ROW_NIL 0x01u
#define IBFT_ROW_BADLEN 0x02u
#define IBFT_ROW_HASH_BAD 0x04u

/* cfg.kernel: how many lanes work on one signature.  The verdicts never depend on it.
 *   AUTO  cold path (recover): TWO wavefronts per signature up to 512 rows (a helper wavefront takes r⁻¹, the scalar split
 *         and u1·G off the critical path), one wavefront per signature up to 2048 rows, one DPP row (16 lanes) per
 *         signature up to 8192 rows, then 4 / 2 lanes per signature while rows*lanes <= 65536, one
 *         lane beyond (the 8-lane form remains selectable);
 *         warm path (known keys): G = 64,32,...,2 lanes per signature so that a batch gives about
 *         one wavefront per SIMD (64 up to 1024 rows), one lane from 65536 rows.
 *   LANE  always one lane per signature (throughput form, both paths).
 *   WAVE  warm path pinned to one wavefront per signature.
 * Experiments only: the environment variable IBFT_COLD_LANES = 1|2|4|8|16|64|128 pins the cold variant (128 = two
 * wavefronts per signature), IBFT_PAIR_ROWS_MAX / IBFT_WAVE_ROWS_MAX / IBFT_ROWS_KERNEL_MAX move the AUTO thresholds of
 * the two-wavefront, the one-wavefront and the row-per-signature forms (read at ibft_ctx_create). */
#define IBFT_KERNEL_AUTO 0u
#define IBFT_KERNEL_LANE 1u
#define IBFT_KERNEL_WAVE 2u

typedef struct ibft_ctx ibft_ctx;

typedef struct {
  int32_t device;    /* HIP device ordinal                                         */
  uint32_t flags;    /* IBFT_FLAG_*                                                 */
  uint32_t max_rows; /* largest batch this context will be asked for (0 = 65536)    */
  uint32_t kernel;   /* IBFT_KERNEL_*                                               */
} ibft_cfg;

typedef struct {
  uint64_t quorum_lo, quorum_hi; /* floor(2*total/3)+1 (validator_manager.go:130-135) */
  uint64_t power_lo, power_hi;   /* Σ power over distinct valid senders ∈ validator set */
  uint32_t valid_rows;           /* popcount of the verdict mask                        */
  uint32_t distinct_senders;     /* distinct member senders among the valid rows        */
  uint32_t has_quorum;           /* power >= quorum                                     */
  uint32_t shard_overlap;        /* sharded calls (ibft_seals_fetch_merged, ibft_group_*): Σ over validators of (shards in which
                                    the validator has a valid row) − 1.  Such a validator is counted ONCE in power and
                                    distinct_senders, like everywhere else; 0 from the single-device calls             */
  uint32_t proposer_rows;        /* HasPrepareQuorum calls (a proposer20 was given): valid rows whose sender IS the proposer —
                                    any such row forces has_quorum = 0 (validator_manager.go:114-121); 0 otherwise     */
  uint32_t reserved;
} ibft_tally_t;

int ibft_version(void);
const char *ibft_strerror(int code);
/* last HIP error string seen by this context (thread-unsafe diagnostic).  ctx = NULL: why the CALLING THREAD's last
 * ibft_ctx_create failed, where the library has a reason to give (IBFT_QTAB_FORM with a value other than wide or glv), else
 * "" — also after a create that succeeded; the string is the thread's own and stays valid until its next ibft_ctx_create. */
const char *ibft_last_error(const ibft_ctx *ctx);

int ibft_ctx_create(const ibft_cfg *cfg, ibft_ctx **out);
void ibft_ctx_destroy(ibft_ctx *ctx);

/* Replace the validator table (addresses n×20, powers n×u64) for `height`.
 * Builds the device-side open-addressing table used for set membership and the
 * weighted tally.  Powers are u64 here (128-bit sums); a set whose powers do not fit
 * uses ibft_set_validators_u256 (validator_manager.go:19 uses *big.Int).           */
int ibft_set_validators(ibft_ctx *ctx, uint64_t height, const uint8_t *addrs20,
                        const uint64_t *power, size_t n);

/* The same with arbitrary-precision powers: ValidatorBackend.GetVotingPowers returns map[string]*big.Int
 * (/root/reference/core/validator_manager.go:17-31) and a stake-weighted set (wei-denominated) exceeds 2^64
 * with ~19 tokens.  power_be32 is n × 32 bytes, each a big-endian 256-bit integer (big.Int.FillBytes of a
 * 32-byte slice); a power that does not fit 256 bits cannot be passed (keep such a set on the Go path).
 * Sums and the quorum ⌊2·total/3⌋+1 are kept in 320 bits; ibft_tally_t then carries the LOW 128 bits of power
 * and quorum and the exact has_quorum flag — ibft_last_tally_wide returns the full-width numbers.          */
int ibft_set_validators_u256(ibft_ctx *ctx, uint64_t height, const uint8_t *addrs20,
                             const uint8_t *power_be32, size_t n);
typedef struct {
  uint64_t quorum[5];        /* little-endian 64-bit words                                     */
  uint64_t power[5];         /* Σ power over distinct valid member senders of the last tally    */
  uint32_t has_quorum, reserved;
} ibft_tally_wide_t;
/* full-width result of the last tally this context delivered (verify / fetch / fetch_merged call)  */
int ibft_last_tally_wide(ibft_ctx *ctx, ibft_tally_wide_t *out);

/* ---- the seal-digest convention ---------------------------------------------------------------------------
 * "IsValidCommittedSeal checks if signature for proposal hash in committed seal is signed by a validator"
 * (/root/reference/core/backend.go:53-55): WHICH bytes the seal signs is the embedding Backend's choice.  Default
 * (IDENTITY): the 32-byte proposalHash itself.  KECCAK_SUFFIX: keccak256(proposalHash ‖ suffix), suffix ≤ 64 bytes —
 * e.g. a Backend that appends the COMMIT message type before hashing passes suffix = {0x02}.  The convention applies to
 * every a2 evaluation of the context: ibft_verify_seals / ibft_seals_stage (the hash32 column still carries the
 * proposalHash each row's message carries; the digest is derived on the device), ibft_wire_stage_seals, the seal half of
 * ibft_verify_messages / ibft_verify_messages_wire (a1 keeps comparing the CARRIED hash with the proposal's), the group
 * calls (ibft_group_set_seal_digest), and ibft_sign_seals (a simulator's seals sign what its verifiers check).  It does
 * not touch a3: an envelope signs keccak256(PayloadNoSig).  Changing it drops a resident staged batch.            */
#define IBFT_SEAL_DIGEST_IDENTITY 0u
#define IBFT_SEAL_DIGEST_KECCAK_SUFFIX 1u
#define IBFT_SEAL_SUFFIX_MAX 64u
int ibft_set_seal_digest(ibft_ctx *ctx, uint32_t mode, const uint8_t *suffix, size_t suffix_len);

/* a1.  raw/raw_len/round: the proposal all rows are checked against.  hash32 is
 * n×32 (zero-filled where absent), hash_len[i] the real byte length (0 = nil).    */
int ibft_verify_hashes(ibft_ctx *ctx, const uint8_t *raw, size_t raw_len, uint64_t round,
                       const uint8_t *hash32, const uint8_t *hash_len, size_t n,
                       uint64_t *out_mask);
/* The same with the proposal's Keccak already in hand (an application Backend computes it when it builds or
 * validates the proposal): a pure 32-byte compare per row.  Recommended for proposals beyond ~64 KiB — Keccak is
 * a sequential sponge, one lane walks it at ≈13 µs per 136-byte block (profiles/r02_a1_sizes.json).         */
int ibft_verify_hashes_digest(ibft_ctx *ctx, const uint8_t digest32[32], const uint8_t *hash32,
                              const uint8_t *hash_len, size_t n, uint64_t *out_mask);
/* keccak256(raw ‖ BE64(round)) (what BuildPrepareMessage's caller would sign).  The context remembers the last
 * proposal it hashed: ibft_verify_hashes / ibft_proposal_hash with the same (raw, round) — every PREPARE and COMMIT set
 * of a round, every wake-up — skip the hash.  WHERE it is hashed: on the calling host thread, with the library's own
 * permutation (csrc/keccak_dev.h compiles for both sides).  Keccak is a sequential sponge — one message cannot be spread
 * over the chip — and one host core absorbs ≈340 MB/s (3.6 µs for 1 KiB, ≈3 ms for 1 MiB) where the one wavefront that
 * can work on it absorbs 25 MB/s (41 ms for 1 MiB, round 2); the 32-byte digest then reaches the device on the side
 * stream, behind the verdict launch it overlaps with.  IBFT_PROPOSAL_HASH=device selects the wavefront kernel (A/B,
 * tests).  The device keeps every hash of which there are MANY to do in parallel: PayloadNoSig of every message, the
 * address of every recovered key, the digests of a certificate tree, the proposals of a batch of blocks
 * (ibft_proposal_hashes below).                                                                                     */
int ibft_proposal_hash(ibft_ctx *ctx, const uint8_t *raw, size_t raw_len, uint64_t round,
                       uint8_t out32[32]);

/* keccak256(a ‖ b) on the host (either part may be empty) — the same routine: for callers that hash what the device
 * hands back (IBFT_CERT_CLASS_DIGEST_BY_HOST rows: a = bytes[0, cut0), b = bytes[cut1, len)).  No context, no device.  */
int ibft_keccak256(const uint8_t *a, size_t na, const uint8_t *b, size_t nb, uint8_t out32[32]);

/* a2.  hash32 n×32 (per-row proposalHash from ExtractCommitHash), sig65 n×65,
 * signer20 n×20 (msg.From).  tally may be NULL.                                   */
int ibft_verify_seals(ibft_ctx *ctx, const uint8_t *hash32, const uint8_t *sig65,
                      const uint8_t *signer20, const uint8_t *pre_flags, size_t n,
                      uint64_t *out_mask, ibft_tally_t *tally);

/* Chain sync: the committed seals of n_blocks finalized blocks, one validator set (the context's), one launch — what a
 * syncing node checks before InsertProposal for every (Proposal, []CommittedSeal) pair it receives
 * (/root/reference/core/backend.go:53-55, 80-82; core/validator_manager.go:77-96).
 *   block_hash32  n_blocks × 32: each block's proposal hash, i.e. what its seals sign (the seal-digest convention of
 *                 ibft_set_seal_digest applies as for ibft_verify_seals)
 *   seal_off      n_blocks + 1, seal_off[0] = 0, non-decreasing: the seals of block b are rows [seal_off[b], seal_off[b+1])
 *   sig65, signer20, pre_flags   one row per seal, as for ibft_verify_seals (pre_flags may be NULL)
 *   out_mask      ⌈n/64⌉ words, n = seal_off[n_blocks]: bit i = IsValidCommittedSeal(block_hash(i), {signer20[i], sig65[i]})
 *   out_tally     n_blocks entries (may be NULL): HasQuorum over the distinct member signers of block b's valid rows
 * Bit for bit what n_blocks separate ibft_verify_seals calls return (each block's hash repeated over its rows): duplicate
 * signers of a block count once, non-members 0, a seal placed in another block than its own is invalid; a block with no
 * rows has has_quorum = 0.  shard_overlap = proposer_rows = 0.  With u256 powers each entry carries the low 128 bits and
 * the exact has_quorum; ibft_last_tally_wide is NOT updated by this call.  IBFT_E_INVAL: NULL ctx or seal_off, seal_off[0]
 * ≠ 0 or decreasing, a NULL column with n > 0; IBFT_E_TOOBIG: n or n_blocks > cfg.max_rows; IBFT_E_NOVALSET.  On return
 * the rows are the resident staged batch, as after ibft_verify_seals; a pipelined pass in flight (ibft_seals_submit) is
 * left to its ibft_seals_collect, as ibft_verify_seals leaves it.                                                      */
int ibft_verify_block_seals(ibft_ctx *ctx, const uint8_t *block_hash32, const uint32_t *seal_off, size_t n_blocks,
                            const uint8_t *sig65, const uint8_t *signer20, const uint8_t *pre_flags,
                            uint64_t *out_mask, ibft_tally_t *out_tally);

/* Streamed chain sync: the batch of ibft_verify_block_seals, submitted and collected in two calls, up to TWO batches in
 * flight — for a node that checks thousands of batches in a row and should not leave the device idle while the host copies
 * verdicts out and pushes the next seals across PCIe.  Per step: submit(k + 1), collect(k).
 *   ibft_block_seals_submit   the arguments and the checks of ibft_verify_block_seals (same codes, same order; a refused call
 *       takes no slot).  Copies the batch into one of two column sets on the context's copy stream, enqueues the kernels
 *       behind that copy and returns WITHOUT waiting for the device.  The caller's buffers must stay untouched until the
 *       collect of this batch has returned.  The copy runs under the kernels of the batch before only from page-locked
 *       sources (ibft_pinned_alloc); pageable sources give the same results, and the submit then lasts as long as the copy.
 *       A batch without rows is a legal batch and takes a slot.  IBFT_E_INVAL (ibft_last_error says which): two batches
 *       already in flight; seal passes of ibft_seals_submit in flight or a batch of ibft_seals_stage_next awaiting its swap —
 *       the two pipelines share their slots and are not mixed (ibft_seals_submit likewise refuses while block batches are in
 *       flight).  A batch is judged under the validator set and the seal-digest convention current at ITS submit.
 *   ibft_block_seals_collect  waits for the OLDEST batch only and delivers what ibft_verify_block_seals would have returned
 *       for it, bit for bit: out_mask ⌈n/64⌉ words (may be NULL only for a batch without rows), out_tally n_blocks entries
 *       (may be NULL).  IBFT_E_INVAL with nothing in flight.  With IBFT_FLAG_PUBKEY_CACHE the tables of the keys the batch
 *       taught the device are built here, after the batch is delivered: that build waits for a newer batch in flight too
 *       (once per cold-to-warm transition), and if it fails the NEXT submit reports it.
 *   ibft_block_seals_pending  batches in flight, rows and blocks of the oldest (0, 0 when none): size out_mask / out_tally
 *       from these.  Any pointer may be NULL.
 * Every other entry point may be called between a submit and its collect: what it enqueues runs behind the batches in
 * flight, which stay collectable (their results wait in their slots); ibft_sync waits for them, ibft_ctx_destroy drops
 * them.  Which form to use (both from pinned sources): from about 16 000 rows per batch on the streamed
 * one (0.96 / 0.88 × the synchronous call's time per batch cold / warm there, 0.87 / 0.72 × at 65 536 rows); up to a few
 * thousand rows a batch is a chain of launch latencies with nothing to hide a copy under, and the synchronous call is as fast. */
int ibft_block_seals_submit(ibft_ctx *ctx, const uint8_t *block_hash32, const uint32_t *seal_off, size_t n_blocks,
                            const uint8_t *sig65, const uint8_t *signer20, const uint8_t *pre_flags);
int ibft_block_seals_collect(ibft_ctx *ctx, uint64_t *out_mask, ibft_tally_t *out_tally);
int ibft_block_seals_pending(ibft_ctx *ctx, uint32_t *batches_in_flight, uint32_t *oldest_rows, uint32_t *oldest_blocks);

/* Bare seals: who signed?  The batch form of ecrecover for committed seals whose signer is not on the wire — finalized headers
 * that store only the 65-byte signatures; an embedder's header check recovers the address, looks it up in the validator
 * set, drops duplicates and asks HasQuorum (/root/reference/core/backend.go:53-55, core/validator_manager.go:77-96).
 *   hash32 n×32 (per-row proposal hash; the ibft_set_seal_digest convention applies as for ibft_verify_seals), sig65 n×65,
 *   pre_flags n or NULL.
 *   out_signer20  n×20: keccak256(X‖Y)[12:32] of the key recovered from row i; TWENTY ZERO BYTES where nothing is
 *                 recovered (r or s out of range, v > 1, no curve point, point at infinity, high s under
 *                 IBFT_FLAG_STRICT_LOW_S) or pre_flags[i] != 0.  A non-member's address is delivered like a member's.
 *   out_vidx      n × int32, may be NULL: index of out_signer20[i] in the context's validator set (the index of its first
 *                 occurrence in the ibft_set_validators list without repeated addresses), -1 when it is no member or nothing
 *                 was recovered
 *   out_mask      ⌈n/64⌉ words: bit i = a key was recovered AND its address is a member
 *                 (= IsValidCommittedSeal(hash_i, {out_signer20[i], sig_i}))
 *   tally         may be NULL: HasQuorum over the distinct member signers of the rows whose bit is set
 * Defining property: out_signer20 fed back as signer20 into ibft_verify_seals with the same other columns returns the same
 * mask words and the same tally, bit for bit, on a cold context and on a warm one.  Always the cold (recovering) kernels,
 * chosen by batch size as for a cold ibft_verify_seals — a warm kernel needs a claimed key to pick its table; with
 * IBFT_FLAG_PUBKEY_CACHE the call teaches the device its validators' keys, so that later VERIFY calls are warm.
 * Errors as ibft_verify_seals (IBFT_E_INVAL: NULL ctx, NULL out_signer20 / out_mask / column with n > 0; IBFT_E_NOVALSET;
 * IBFT_E_TOOBIG); nothing is written to the out buffers of a refused call; n = 0 is legal.  Towards the two pipelines as
 * ibft_verify_seals: what it enqueues runs behind batches in flight, a pass in flight is left to its collect.  Bare rows are
 * NOT a resident staged batch afterwards (ibft_seals_launch finds no rows).  ibft_last_dispatch, ibft_last_kernel_ms and
 * ibft_set_kernel_timing see the call as a cold verify pass.                                                          */
int ibft_recover_seals(ibft_ctx *ctx, const uint8_t *hash32, const uint8_t *sig65, const uint8_t *pre_flags, size_t n,
                       uint8_t *out_signer20, int32_t *out_vidx, uint64_t *out_mask, ibft_tally_t *tally);

/* The same for n_blocks finalized blocks in one launch: arguments, checks and error codes of ibft_verify_block_seals minus
 * the signer20 column, plus out_signer20 (n×20, NULL with n > 0: IBFT_E_INVAL) and out_vidx (n, may be NULL); out_tally
 * n_blocks entries, may be NULL.  Equal to one ibft_recover_seals per block: a signer counts once per block, in every block
 * it signed; a seal placed in another block recovers some other address and counts only if that address is a member.
 * Streamed form: ibft_recover_block_seals_submit, below the _raw calls.                                                */
int ibft_recover_block_seals(ibft_ctx *ctx, const uint8_t *block_hash32, const uint32_t *seal_off, size_t n_blocks,
                             const uint8_t *sig65, const uint8_t *pre_flags,
                             uint8_t *out_signer20, int32_t *out_vidx, uint64_t *out_mask, ibft_tally_t *out_tally);

/* Chain sync from the PROPOSALS.  A node that is catching up holds (Proposal, []CommittedSeal) pairs
 * (/root/reference/core/backend.go:80-82, messages/helpers.go:16-35), not proposal hashes: what the seals of a block sign is
 * keccak256(RawProposal ‖ BE64(Round)) and the node has to COMPUTE it — a hash a peer sends along is evidence of nothing.
 * One sponge is sequential (ibft_proposal_hash: on the host); the hashes of a batch of blocks are MANY, so they are the device's.
 *   raw       the proposals' RawProposal bytes, concatenated — as they are: nothing is padded, aligned or re-packed
 *   raw_off   n + 1 offsets, raw_off[0] = 0, non-decreasing: proposal i is raw[raw_off[i], raw_off[i+1]) (any length, 0 included)
 *   round     n: Proposal.Round of each
 *   out_hash32[32·i …] = keccak256(raw_i ‖ BE64(round[i]))
 * Defining property: row i equals ibft_proposal_hash(ctx, raw_i, len_i, round[i]) byte for byte, for every length, in both forms
 * of the kernel — one lane per proposal (throughput) or one wavefront per proposal (latency), chosen by batch shape: the lane
 * form from 8 192 proposals of the longest one's length on (total rate blocks ≥ 8 192 × the longest proposal's; environment
 * IBFT_PROPOSAL_LANE_ROWS moves that, IBFT_PROPOSAL_LANES = 1|64 pins a form; both read at ibft_ctx_create).
 * The call neither reads nor changes the proposal the context remembers (ibft_proposal_hash / ibft_verify_hashes /
 * ibft_forget_proposal work as before), needs no validator set and leaves a resident staged batch alone; n = 0 is legal (no
 * pointer is looked at).  Sources in ibft_pinned_alloc memory are read by one gather launch, pageable ones by a copy command
 * per column; the results are the same.  Checked in this order: IBFT_E_INVAL NULL ctx, NULL out_hash32 / raw_off / round with
 * n > 0, raw_off[0] ≠ 0; IBFT_E_TOOBIG n > cfg.max_rows; IBFT_E_INVAL decreasing offsets; IBFT_E_TOOBIG raw_off[n] above the
 * byte budget (environment IBFT_PROPOSAL_BYTES_MAX, default 256 MiB = 268435456; the device buffer grows on demand up to it and
 * is kept); IBFT_E_INVAL NULL raw with raw_off[n] > 0.  Nothing is written to out_hash32 by a refused call.  From which proposal
 * size on a caller with idle cores should hash on the host instead: INTEGRATION.md §11.                                   */
int ibft_proposal_hashes(ibft_ctx *ctx, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round, size_t n,
                         uint8_t *out_hash32);

/* ibft_verify_block_seals / ibft_recover_block_seals with the PROPOSALS of the n_blocks blocks (raw, raw_off, round as for
 * ibft_proposal_hashes with n = n_blocks) in place of block_hash32: the hashes are computed on the device and never cross
 * PCIe on the way in.  out_block_hash32: n_blocks × 32, may be NULL — the computed proposal hashes (BEFORE the seal-digest
 * convention is applied), for the caller's own IsValidProposalHash compare of 32 bytes.
 * Defining property: the call equals ibft_proposal_hashes followed by the hashes-given call with those hashes — same mask
 * words, tallies, signer / index columns, bit for bit, cold and warm, under every convention of ibft_set_seal_digest (applied
 * to the computed hash exactly as to a given one).  Everything the hashes-given calls document holds unchanged: the rows are
 * the resident staged batch after the verify form and not after the recover form, behaviour towards the two pipelines, key
 * learning.  Errors: those of the hashes-given call in its order (minus the NULL block_hash32), then those of
 * ibft_proposal_hashes' arguments in its order; nothing is written to any out buffer of a refused call.  With no seal rows at
 * all the proposals are hashed only if out_block_hash32 is given.  Streamed forms: ibft_block_seals_submit_raw and
 * ibft_recover_block_seals_submit_raw, below.                                                                              */
int ibft_verify_block_seals_raw(ibft_ctx *ctx, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                const uint32_t *seal_off, size_t n_blocks, const uint8_t *sig65, const uint8_t *signer20,
                                const uint8_t *pre_flags, uint8_t *out_block_hash32, uint64_t *out_mask,
                                ibft_tally_t *out_tally);
int ibft_recover_block_seals_raw(ibft_ctx *ctx, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                 const uint32_t *seal_off, size_t n_blocks, const uint8_t *sig65, const uint8_t *pre_flags,
                                 uint8_t *out_block_hash32, uint8_t *out_signer20, int32_t *out_vidx, uint64_t *out_mask,
                                 ibft_tally_t *out_tally);

/* Streamed chain sync FROM THE PROPOSALS and FROM BARE SEALS: the submit / collect pipeline of ibft_block_seals_submit with
 * the reach of the synchronous calls.  A syncer streams the (Proposal, []CommittedSeal) pairs it holds — no synchronous
 * ibft_proposal_hashes between two submits, which would wait for the batches in flight — and a chain whose headers carry
 * only 65-byte signatures streams too.
 *   ibft_block_seals_submit_raw          sibling: ibft_verify_block_seals_raw
 *   ibft_recover_block_seals_submit      sibling: ibft_recover_block_seals
 *   ibft_recover_block_seals_submit_raw  sibling: ibft_recover_block_seals_raw
 * Defining property: each submit, collected with ibft_block_seals_collect_ex, delivers bit for bit what its synchronous
 * sibling returns for the same arguments — mask words, every field of every ibft_tally_t, out_signer20, out_vidx and
 * out_block_hash32 (the hashes BEFORE the seal-digest convention) — cold and warm, under every ibft_set_seal_digest convention,
 * with IBFT_FLAG_STRICT_LOW_S on and off, for u64 and u256 powers, in both forms of the digest kernel.
 * Rules:
 *  - Argument checks: those of the synchronous sibling, in the sibling's order, minus the out buffers; then the pipeline's
 *    refusals as ibft_block_seals_submit documents them (IBFT_E_INVAL: two batches in flight, seal passes in flight, a staged
 *    batch awaiting its swap; the code of a deferred table-build error).  A refused call takes no slot.
 *  - Shared slots: the three submits share the two slots with ibft_block_seals_submit.  Batches of different kinds may be in
 *    flight together; they are collected oldest first; ibft_block_seals_pending counts them all.
 *  - Pinned state: a batch is judged under the validator set, the seal-digest convention and the form of the digest kernel
 *    current at ITS submit.
 *  - Caller buffers: sig65, signer20, pre_flags, seal_off, block_hash32 and raw / raw_off / round stay untouched until the
 *    collect of that batch has returned.  Pageable sources give the same results without the overlap, as for
 *    ibft_block_seals_submit.
 *  - Device memory: each of the two slots keeps the proposals of its batch (grown on demand, each slot bounded by
 *    IBFT_PROPOSAL_BYTES_MAX): two slots DOUBLE the device bytes proposals can take.
 *  - ibft_block_seals_collect_ex waits for the OLDEST batch, whatever its kind.  out_mask and out_tally as in
 *    ibft_block_seals_collect.  out_block_hash32 (n_blocks × 32) may be NULL and is written only for a batch with
 *    IBFT_BATCH_RAW; with no seal rows at all the proposals are hashed only if the batch was submitted raw, and the hashes
 *    are then delivered if asked for.  out_signer20 (n × 20) must be non-NULL for a recover batch with rows: IBFT_E_INVAL
 *    otherwise, the batch stays in flight and nothing is written.  out_vidx (n) may be NULL.  For a verify batch out_signer20
 *    and out_vidx are not written.
 *  - ibft_block_seals_collect (the old call): a verify batch submitted raw is collected normally, its hashes are dropped; a
 *    recover batch with rows gets IBFT_E_INVAL, stays in flight and ibft_last_error names ibft_block_seals_collect_ex; batches
 *    of ibft_block_seals_submit as before.
 *  - Resident rows: after a verify-kind submit the rows are the resident staged batch, as after ibft_block_seals_submit; after
 *    a recover-kind submit they are not (ibft_seals_launch finds no rows), as after the synchronous siblings.
 *  - Key cache: a recover batch teaches keys; tables are built at its collect, as for the batches of ibft_block_seals_submit,
 *    and a failed build is reported by the next submit of any kind.
 *  - ibft_sync, ibft_ctx_destroy and every other entry point behave towards these batches as towards those of
 *    ibft_block_seals_submit.
 *  - ibft_block_seals_pending_ex: ibft_block_seals_pending plus the kind of the oldest batch (IBFT_BATCH_* bits, 0 for a batch
 *    of ibft_block_seals_submit and when none is in flight).  Any pointer may be NULL.
 * Where the digests are computed: environment IBFT_STREAM_DIGEST=copy|main, read at ibft_ctx_create — `copy` puts
 * proposal_digest_kernel of batch k + 1 on the copy stream behind the copy of its bytes, next to the verdict kernel of batch
 * k; `main` puts it on the main stream in front of its own batch's kernels.  Results are the same bits.  The default is
 * `main`: the A/B of the two placements (tools/block_seals_stream_raw_rate.py) HAS NOT BEEN RUN on a device, and no gain of
 * the streamed raw / recover forms over the synchronous calls is claimed.                               */
#define IBFT_BATCH_RECOVER 1u /* bit 0 of a batch's kind: bare seals, signers are emitted */
#define IBFT_BATCH_RAW 2u     /* bit 1: proposals were given, hashes are computed and can be delivered */
#define IBFT_BATCH_SETS 4u    /* bit 2: judged under a set per block (the _sets submits, below the family's calls) */
int ibft_block_seals_submit_raw(ibft_ctx *ctx, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                const uint32_t *seal_off, size_t n_blocks, const uint8_t *sig65, const uint8_t *signer20,
                                const uint8_t *pre_flags);
int ibft_recover_block_seals_submit(ibft_ctx *ctx, const uint8_t *block_hash32, const uint32_t *seal_off, size_t n_blocks,
                                    const uint8_t *sig65, const uint8_t *pre_flags);
int ibft_recover_block_seals_submit_raw(ibft_ctx *ctx, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                        const uint32_t *seal_off, size_t n_blocks, const uint8_t *sig65,
                                        const uint8_t *pre_flags);
int ibft_block_seals_collect_ex(ibft_ctx *ctx, uint8_t *out_block_hash32, uint8_t *out_signer20, int32_t *out_vidx,
                                uint64_t *out_mask, ibft_tally_t *out_tally);
int ibft_block_seals_pending_ex(ibft_ctx *ctx, uint32_t *batches_in_flight, uint32_t *oldest_rows, uint32_t *oldest_blocks,
                                uint32_t *oldest_kind);

/* Chain sync ACROSS validator-set changes: a FAMILY of validator sets on the context, and block calls that judge every
 * block under the set the caller names for it — one call, one verdict launch, whatever the sets do between the blocks.
 * A syncer collects the distinct sets of the run it fetched (GetVotingPowers per height), installs them once and passes
 * block_set[b]; it no longer cuts its batch where the set changes.
 *
 * ibft_set_validator_sets[_u256]: n_sets sets; set s is entries [set_off[s], set_off[s+1]) of addrs20 / power (set_off has
 *   n_sets + 1 entries, set_off[0] = 0, non-decreasing).  height[s]: informational, as in ibft_set_validators; may be NULL.
 *   Within a set a repeated address keeps its LAST power and its FIRST position, exactly as ibft_set_validators treats its
 *   list; the index of an address in set s (out_vidx below) is the index ibft_set_validators(set s) would give it.
 *   The library builds one lookup table over the UNION of the family's addresses, a dense n_sets × union table of int32
 *   (the index of union address u in set s, or −1) and per-set powers, quorum and size.
 *   Checked in this order: IBFT_E_INVAL NULL ctx, n_sets = 0, NULL set_off, set_off[0] ≠ 0, decreasing offsets, a NULL column
 *   with entries; IBFT_E_TOOBIG a set's list or the union holds more than cfg.max_rows addresses, or the family's device
 *   tables exceed the byte budget (environment IBFT_VALSETS_BYTES_MAX, read at ibft_ctx_create; default 512 MiB =
 *   536870912: 1 024 sets over a union of 8 192 take 32 MiB for the dense table and at most 64 MiB (u64) / 256 MiB (u256)
 *   of powers); IBFT_E_POWER when ANY set's total power is zero, an empty set included.  All of it is decided on the host.
 *   Installing a family replaces the previous family whole; a refused install leaves the previous one in place.
 * ibft_validator_sets_info: sets and union addresses of the installed family and the device bytes it holds now (0, 0, 0
 *   without one): the CAPACITIES of its buffers — the tables the budget counts (there by their computed sizes; a buffer is
 *   never smaller than 256 bytes), plus the key-cache slot column of the union and the block_set columns the _sets calls
 *   upload (one for the synchronous calls, one per slot of the streamed ones), which grow with their n_blocks and are not
 *   part of the budget.  Any pointer may be NULL.
 *
 * ibft_verify_block_seals_sets / ibft_recover_block_seals_sets: ibft_verify_block_seals / ibft_recover_block_seals plus
 *   block_set (n_blocks entries, each < n_sets): the set block b is judged under.
 * Defining property: for every block b the mask bits of its rows, its ibft_tally_t (all fields; quorum_* is the quorum of
 * set block_set[b]) and, in the recover form, its out_signer20 / out_vidx rows are bit for bit what
 * ibft_set_validators(set block_set[b]) followed by ibft_verify_seals / ibft_recover_seals over that block's rows returns —
 * cold and warm, under every ibft_set_seal_digest convention, with IBFT_FLAG_STRICT_LOW_S on and off, for u64 and u256
 * powers (low 128 bits and the exact has_quorum, as the block calls document; ibft_last_tally_wide is not updated).  A block
 * without rows has has_quorum = 0 and its set's quorum.  A validator that is in the family but not in the block's set gets
 * bit 0 and no power in that block, and out_vidx −1 — its address in out_signer20 is delivered like any non-member's.
 * Rules:
 *  - The family is separate state.  ibft_set_validators and every other entry point neither read nor change it and behave
 *    exactly as without one; the _sets calls never read the context's single set and do not need one: IBFT_E_NOVALSET
 *    from them means "no family installed".
 *  - Errors: those of ibft_verify_block_seals / ibft_recover_block_seals in their order; IBFT_E_INVAL for a NULL block_set
 *    with n_blocks > 0 (with the NULL columns) and, behind IBFT_E_NOVALSET, for an entry ≥ n_sets — decided on the host,
 *    before anything is launched.  Nothing is written to any out buffer of a refused call.
 *  - After a _sets call the rows are NOT a resident staged batch (as after the recover forms: ibft_seals_launch finds no
 *    rows).  Towards the two pipelines the calls behave as ibft_verify_block_seals does.  ibft_last_dispatch,
 *    ibft_last_kernel_ms and ibft_cache_stats see a normal verify pass; the AUTO rule sees the total row count.
 *  - Key cache (IBFT_FLAG_PUBKEY_CACHE): the union's addresses hold key-cache slots while the family is installed (the family
 *    counts as a referrer of a slot next to the contexts' single sets: ibft_cache_memory); a _sets verify call teaches keys,
 *    and later calls — _sets or single-set, on this context or another of the device — are warm for those addresses.  A
 *    signer in the union but not in its block's set is verified like any row and its bit then cleared: the verdict (0) of
 *    the per-set call's non-member early-out.
 *  - The install calls (ibft_set_validator_sets[_u256]) are synchronous: there is
 *    no streamed (submit / collect) form of these calls.  They may be called with _sets batches in flight (below).
 *
 * FROM THE PROPOSALS — ibft_verify_block_seals_sets_raw / ibft_recover_block_seals_sets_raw: the _sets calls with raw /
 *   raw_off / round in the place of block_hash32, as ibft_verify_block_seals_raw has them.  Defining property: each equals
 *   ibft_proposal_hashes followed by the hashes-given _sets call with those hashes — mask words, every field of every
 *   ibft_tally_t, out_signer20, out_vidx and out_block_hash32 (the hashes BEFORE the seal-digest convention), cold and warm,
 *   in both forms of the digest kernel, under every convention, strict-low-s on and off, u64 and u256 families.  Errors:
 *   those of the hashes-given _sets call in its order, minus the NULL block_hash32; then those of ibft_proposal_hashes'
 *   arguments in its order.  A refused call writes nothing.  With no seal rows at all the proposals are hashed only if
 *   out_block_hash32 is given.
 *
 * STREAMED — the submit / collect pipeline of ibft_block_seals_submit, a set per block:
 *   ibft_block_seals_submit_sets              sibling: ibft_verify_block_seals_sets
 *   ibft_block_seals_submit_sets_raw          sibling: ibft_verify_block_seals_sets_raw
 *   ibft_recover_block_seals_submit_sets      sibling: ibft_recover_block_seals_sets
 *   ibft_recover_block_seals_submit_sets_raw  sibling: ibft_recover_block_seals_sets_raw
 *   Collected with ibft_block_seals_collect[_ex]; ibft_block_seals_pending_ex reports IBFT_BATCH_SETS in oldest_kind.
 *   Defining property: each submit, collected with ibft_block_seals_collect_ex, delivers bit for bit what its synchronous
 *   sibling returns for the same arguments under the family that was installed at the submit.
 *  - Pinned state: a sets batch is judged under the family, the seal-digest convention and the digest-kernel form current at
 *    ITS submit.  ibft_set_validator_sets[_u256] between a submit and its collect is legal and does not change that batch:
 *    set membership, out_vidx and the quorum_* fields of its tallies are the old family's.  The install waits for the kernels
 *    of the batches in flight before the old family's device tables are released and before the key-cache references of the
 *    old union are dropped; the batches' results already sit in their slots and stay collectable.  A refused install leaves
 *    the family and the batches untouched.
 *  - Shared slots: the four submits share the two slots with the four single-set submits; batches of any kinds may be in
 *    flight together (a single-set batch between two sets batches) and are collected oldest first.  A single-set batch is
 *    judged under the single set, a sets batch under the family; each needs only its own kind of set: IBFT_E_NOVALSET from a
 *    sets submit means "no family installed", and a single-set submit with only a family installed keeps returning it.
 *  - Checks: the synchronous sibling's, in its order, minus the out buffers — the NULL block_set with n_blocks > 0 and,
 *    behind IBFT_E_NOVALSET, an entry ≥ n_sets included, both decided on the host —; then the pipeline's refusals.  A refused
 *    call takes no slot and enqueues nothing.
 *  - Caller buffers: block_set stays untouched until the collect of its batch has returned, like every other column.
 *  - After a sets submit the rows are not a resident staged batch.  Key learning and the table build at the collect work as
 *    for the other submits, over the union's slots.  ibft_sync, ibft_ctx_destroy, ibft_block_seals_pending and every other
 *    entry point behave as towards any batch in flight.  ibft_block_seals_collect (the old call) treats a sets verify batch
 *    like any verify batch and refuses a sets recover batch with rows, as it refuses any recover batch.
 *  - Device memory: each slot keeps the block_set column of its batch (4 bytes per block, in ibft_validator_sets_info's
 *    device_bytes); the collect's quorum words are kept on the host.
 *
 * Which form to use: a run judged under ONE set — the single-set calls, which do without the per-row load of the dense
 * table and one upload.  A run that crosses set changes — the _sets calls; from proposals, the _sets_raw calls; a syncer
 * that keeps batches in flight, the _sets submits, installing the next run's family while the last batches of this run are
 * still in flight.  MEASURED (tools/block_seals_sets_stream_rate.py, V = 100, a set change every 64 blocks, 1 KiB proposals,
 * pinned sources; profiles/r23_block_seals_sets_stream_rate.txt): per batch the streamed sets form with one batch in flight
 * takes 0.84 × (cold) / 0.95 × (warm) the time of ibft_proposal_hashes + ibft_verify_block_seals_sets at 65 500 rows, and
 * 1.00 × / 1.02 × at 16 300 rows — it pays from batches of several ten thousand rows on and not below; against batches cut
 * at every set change and streamed under ibft_set_validators it takes 0.13 … 0.16 × at 65 500 rows and 0.36 … 0.45 × at 16 300.
 * What the _sets call gains over a cut batch and what it costs over the single-set call: DESIGN.md §5.11.
 * Out of scope: streamed (submit / collect) forms over a device group, the sharded group calls as a whole, appending to a
 * family in place, more than two batches in flight, and a family for the message-set and certificate entry points.  (The
 * live route is NOT out of scope: IsValidValidator is defined per message, against the validators at the height IN the
 * message, and a node stores the messages of heights ahead of its own — ibft_verify_senders_wire_sets, further down.)  */
int ibft_set_validator_sets(ibft_ctx *ctx, size_t n_sets, const uint64_t *height, const uint32_t *set_off,
                            const uint8_t *addrs20, const uint64_t *power);
int ibft_set_validator_sets_u256(ibft_ctx *ctx, size_t n_sets, const uint64_t *height, const uint32_t *set_off,
                                 const uint8_t *addrs20, const uint8_t *power_be32);
int ibft_validator_sets_info(ibft_ctx *ctx, uint32_t *n_sets, uint32_t *union_size, uint64_t *device_bytes);
int ibft_verify_block_seals_sets(ibft_ctx *ctx, const uint8_t *block_hash32, const uint32_t *seal_off,
                                 const uint32_t *block_set, size_t n_blocks, const uint8_t *sig65,
                                 const uint8_t *signer20, const uint8_t *pre_flags, uint64_t *out_mask,
                                 ibft_tally_t *out_tally);
int ibft_recover_block_seals_sets(ibft_ctx *ctx, const uint8_t *block_hash32, const uint32_t *seal_off,
                                  const uint32_t *block_set, size_t n_blocks, const uint8_t *sig65,
                                  const uint8_t *pre_flags, uint8_t *out_signer20, int32_t *out_vidx,
                                  uint64_t *out_mask, ibft_tally_t *out_tally);
int ibft_verify_block_seals_sets_raw(ibft_ctx *ctx, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                     const uint32_t *seal_off, const uint32_t *block_set, size_t n_blocks,
                                     const uint8_t *sig65, const uint8_t *signer20, const uint8_t *pre_flags,
                                     uint8_t *out_block_hash32, uint64_t *out_mask, ibft_tally_t *out_tally);
int ibft_recover_block_seals_sets_raw(ibft_ctx *ctx, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                      const uint32_t *seal_off, const uint32_t *block_set, size_t n_blocks,
                                      const uint8_t *sig65, const uint8_t *pre_flags, uint8_t *out_block_hash32,
                                      uint8_t *out_signer20, int32_t *out_vidx, uint64_t *out_mask,
                                      ibft_tally_t *out_tally);
int ibft_block_seals_submit_sets(ibft_ctx *ctx, const uint8_t *block_hash32, const uint32_t *seal_off,
                                 const uint32_t *block_set, size_t n_blocks, const uint8_t *sig65,
                                 const uint8_t *signer20, const uint8_t *pre_flags);
int ibft_block_seals_submit_sets_raw(ibft_ctx *ctx, const uint8_t *raw, const uint32_t *raw_off, const uint64_t *round,
                                     const uint32_t *seal_off, const uint32_t *block_set, size_t n_blocks,
                                     const uint8_t *sig65, const uint8_t *signer20, const uint8_t *pre_flags);
int ibft_recover_block_seals_submit_sets(ibft_ctx *ctx, const uint8_t *block_hash32, const uint32_t *seal_off,
                                         const uint32_t *block_set, size_t n_blocks, const uint8_t *sig65,
                                         const uint8_t *pre_flags);
int ibft_recover_block_seals_submit_sets_raw(ibft_ctx *ctx, const uint8_t *raw, const uint32_t *raw_off,
                                             const uint64_t *round, const uint32_t *seal_off, const uint32_t *block_set,
                                             size_t n_blocks, const uint8_t *sig65, const uint8_t *pre_flags);

/* a3. payload = concatenated PayloadNoSig bytes; row i is payload[off[i]..off[i+1]);
 * off has n+1 entries.                                                             */
int ibft_verify_senders(ibft_ctx *ctx, const uint8_t *payload, const uint32_t *off,
                        const uint8_t *sig65, const uint8_t *from20, const uint8_t *pre_flags,
                        size_t n, uint64_t *out_mask, ibft_tally_t *tally);

/* ---- the wire bytes themselves ---------------------------------------
 * Rows are IbftMessage protobuf bytes as the transport delivers them
 * (/root/reference/messages/proto/messages.proto:24-44); row i is wire[off[i]..off[i+1]).
 * Replaces, for PREPARE and COMMIT messages, the host's proto.Unmarshal + PayloadNoSig re-marshal
 * (/root/reference/messages/proto/helper.go:12-27) + column flattening in front of a3: the device
 * walks the fields, vouches that the bytes are the canonical encoding (so that "wire minus the
 * signature field" IS PayloadNoSig), hashes them, extracts From / Signature / view / proposal hash
 * / committed seal and verifies the sender.  out_rows (n entries, may be NULL) tells the host what
 * was found.  A row with status IBFT_WIRE_NEEDS_HOST (PREPREPARE / ROUND_CHANGE payloads, unknown
 * fields, any non-canonical encoding, truncated input) is NOT judged: its verdict bit is 0 and the
 * caller must decode it with the protobuf runtime and use ibft_verify_senders.
 *
 * THE RECODE CLASS (IBFT_FLAG_WIRE_RECODE; csrc/wire_recode_dev.h).  The reference signs proto.Marshal of the DECODED
 * message with its signature cleared, so a PREPARE / COMMIT message in another encoding is as valid as the canonical one,
 * and anybody who can reach the transport could otherwise push a whole round onto the per-message host route.  With the
 * flag on, both flat wire calls run a second walk over the rows the canonical walk marked NEEDS_HOST, before the verdict
 * launch and on the same stream.  A row in the class is decoded tolerantly, its canonical PayloadNoSig is hashed on the
 * device, and EVERY output of the call — masks, rows, classes, tally, the columns ibft_wire_stage_seals reads — is what
 * the flag-off call returns for the same batch with that row replaced by its canonical re-encoding (the message
 * re-marshalled, signature kept).  The one exception: ibft_wire_row_t.pad[0] is 1 for such a row.  A row outside the class
 * keeps NEEDS_HOST and verdict 0, exactly as without the flag.  The rule, at each of the three levels of a flat message
 * (IbftMessage, View, the PrepareMessage / CommitMessage body):
 *   - every tag is ONE byte and names a field of that message with that field's wire type — IbftMessage: 1, 2, 3, 6, 7
 *     LEN, 4 VARINT; View: 1, 2 VARINT; body: 1 LEN, and 2 LEN in a CommitMessage only.  Field 5 or 8 anywhere in the
 *     message, any other field number, a wrong wire type, a multi-byte tag: NEEDS_HOST;
 *   - varints may be padded: VALUES are 1 to 10 bytes (a tenth byte above 1 or an eleventh byte: NEEDS_HOST), LENGTH
 *     PREFIXES 1 to 5 bytes (a sixth byte: NEEDS_HOST — protobuf runtimes differ there: upb refuses a longer prefix, Go's
 *     protowire takes ten); a length that leaves its enclosing message: NEEDS_HOST;
 *   - fields come in any order and any number of times.  For a scalar or bytes field the last occurrence wins;
 *     occurrences of View merge, per field the last wins, and a present but empty View is kept (0a 00); an occurrence of
 *     the other oneof member discards what the earlier member held, a further occurrence of the same member merges into
 *     it;
 *   - explicit zero scalars and empty byte strings are defaults and vanish in the re-encoding; an empty signature is no
 *     signature;
 *   - after decoding, the canonical walk's own limits: type <= 255 (of the decoded 64-bit value, not truncated), proposal
 *     hash <= 32 bytes; otherwise NEEDS_HOST.
 * Unknown fields stay out of the class although Go re-emits them behind the known ones; the restrictions above are where
 * decoders may differ.                                                                           */
#define IBFT_WIRE_OK 0u
#define IBFT_WIRE_NEEDS_HOST 1u
typedef struct {
  uint64_t height, round;    /* View (0 when absent / omitted)                              */
  uint8_t status;            /* IBFT_WIRE_*                                                  */
  uint8_t type;              /* IbftMessage.type                                             */
  uint8_t payload_kind;      /* oneof member: 0 none, 6 PrepareMessage, 7 CommitMessage (5 PrePrepareMessage,
                                8 RoundChangeMessage: ibft_verify_certificates_wire only)    */
  uint8_t has_view;
  uint8_t hash_len;          /* bytes of proposal_hash present (<= 32)                       */
  uint8_t seal_len;          /* bytes of committed_seal present (255 = more)                 */
  uint8_t from_len, sig_len; /* 255 = more                                                   */
  uint8_t from[20];
  uint8_t proposal_hash[32];
  uint8_t pad[4];            /* the first byte is `recoded`: 1 when the row was judged through the recode class
                                (IBFT_FLAG_WIRE_RECODE), else 0; the other three are 0          */
} ibft_wire_row_t;
int ibft_verify_senders_wire(ibft_ctx *ctx, const uint8_t *wire, const uint32_t *off, size_t n,
                             uint64_t *out_mask, ibft_wire_row_t *out_rows, ibft_tally_t *tally);
/* Make the COMMIT seals found by the last ibft_verify_senders_wire the resident seal batch
 * (hash column <- proposal hash, signature column <- committed seal, signer <- From): follow with
 * ibft_seals_launch + ibft_seals_fetch — a2 without another upload.  Rows that are not canonical
 * COMMIT messages (type COMMIT, 32-byte hash, 65-byte seal, 20-byte From) are pre-flagged.      */
int ibft_wire_stage_seals(ibft_ctx *ctx);
/* What the walks made of the rows of the LAST flat wire call of the context that succeeded (ibft_verify_senders_wire or
 * ibft_verify_messages_wire): rows = n; recoded_rows = rows judged through the recode class (pad[0] = 1; always 0 without
 * IBFT_FLAG_WIRE_RECODE); needs_host_rows = rows left IBFT_WIRE_NEEDS_HOST.  Counted when asked, from the parse results
 * still on the device (one copy of 80 bytes per row: a diagnostic, not for the hot path).  Any pointer may be NULL; a NULL
 * ctx: IBFT_E_INVAL; all zero before the first such call or after a certificate call has reused the rows.  No new
 * ibft_version(): a build without the symbol simply lacks it.                                                        */
int ibft_wire_stats(ibft_ctx *ctx, uint32_t *rows, uint32_t *recoded_rows, uint32_t *needs_host_rows);

/* ---- the wire route under a FAMILY of sets: every message judged under the validator set of ITS OWN height -------------
 * IsValidValidator asks whether "the signer address is one of the validators at the height in message"
 * (core/backend.go:41-45), and IBFT.AddMessage accepts — and stores for later — every message of the node's own height OR
 * A GREATER ONE (core/ibft.go:1126-1149), dropping for good what IsValidValidator rejects.  On a chain whose validator set
 * moves at an epoch boundary a node one block behind therefore receives PREPAREs and COMMITs of height h + 1 while it runs
 * h, at every height: under the one set of ibft_verify_senders_wire a validator that joins at h + 1 is rejected (its
 * message is lost) and one that left is accepted, unless the caller cuts every receive-queue batch by height and pays an
 * ibft_set_validators per piece.  With the validator-set family (ibft_set_validator_sets, above) and a map from heights to
 * its sets, the batch goes in whole.
 *
 * ibft_set_height_sets: heights in [first_height[k], first_height[k+1]) are judged under set range_set[k] of the installed
 *   family (first_height has n_ranges + 1 entries, strictly increasing; adjacent ranges may name the same set); every other
 *   height has no set.  Checked in this order: IBFT_E_INVAL NULL ctx; n_ranges = 0 clears the map and returns IBFT_OK;
 *   IBFT_E_INVAL NULL first_height / range_set, or heights that are not strictly increasing; IBFT_E_TOOBIG n_ranges above
 *   IBFT_HEIGHT_RANGES_MAX; IBFT_E_NOVALSET no family installed; IBFT_E_INVAL an entry of range_set >= n_sets.
 *   A refused install leaves the old map in place.  Installing a family (ibft_set_validator_sets[_u256]) DROPS the map — its indices
 *   named sets of the old family — behind the same wait for work in flight that lets the old family go; install the map
 *   again after every family.  The map is two small device tables; the call also sizes and zeroes the per-set scratch of
 *   the tally (8 bytes × (2 · power words + 1) per set, one bit per (set, member)) and waits for the context's stream.
 * ibft_height_sets_info: ranges of the installed map, its first mapped height (lo) and the first height past its last
 *   range (hi); 0, 0, 0 without a map.  Any pointer may be NULL; IBFT_E_INVAL for a NULL ctx.
 *
 * ibft_verify_senders_wire_sets: ibft_verify_senders_wire for a batch that mixes heights.  out_rows, out_set, out_vidx
 *   (n entries each) and out_tally (n_sets entries, one per set of the family) may be NULL.
 * Row rule: out_set[i] is the map's set for the height the walk decoded for row i, and −1 when the walks left the row
 *   IBFT_WIRE_NEEDS_HOST, when the message has no View, or when its height is in no range.  A View that is present but empty
 *   has height 0 and is mapped like any height.  With IBFT_FLAG_WIRE_RECODE the recoded row's height counts.  A row with
 *   set −1 has verdict bit 0 and out_vidx −1 and is counted in no tally; it is
 *   pre-flagged on the device IN FRONT of the verdict launch, so a peer that sprays far-future heights buys no ECDSA work.
 * Defining property: for every set s, with R_s the subsequence of rows with out_set == s, the mask bits of those rows and
 *   out_tally[s] (every field; quorum_* is the quorum of set s) are bit for bit what ibft_set_validators(set s) followed by
 *   ibft_verify_senders_wire(R_s) returns; out_vidx is the index ibft_set_validators(set s) would give the sender, −1 where
 *   the bit is 0 — cold and warm (IBFT_FLAG_PUBKEY_CACHE), for u64 and u256 families (low 128 bits of the power and the exact
 *   has_quorum, as the block calls; ibft_last_tally_wide is not updated), with IBFT_FLAG_WIRE_RECODE on and off.  A set
 *   without rows has its own quorum, zero counts and has_quorum = 0.  out_rows is what ibft_verify_senders_wire delivers
 *   for the whole batch.  A sender in the union but not in its row's set is verified like any row and then loses its bit:
 *   the rule of the block _sets calls.
 * Errors: those of ibft_verify_senders_wire in its order, except that IBFT_E_NOVALSET means
 *   "no family installed or no height map installed".  A call that fails with a device or
 *   allocation error after its checks drops the height map (its scratch may be half used): install the map again.  The call never reads the context's single set and does not need one.  A refused call writes
 *   nothing to any out buffer.
 * Afterwards the rows are NOT a resident staged batch (ibft_seals_launch finds no rows), and
 *   ibft_wire_stage_seals answers IBFT_E_INVAL, as it does whenever no senders-wire batch is resident: the columns hold verdicts against the union,
 *   nothing the single-set seal pass could continue from.  ibft_wire_stats reports on this call like on any flat wire call.
 *   Towards the two pipelines, ibft_last_dispatch, ibft_last_kernel_ms and the key cache the call behaves as
 *   ibft_verify_senders_wire does (keys are learned over the union's slots, as by the block _sets calls).  No new
 *   ibft_version(): a build without the symbols simply lacks them.
 * MEASURED (tools/wire_sets_rate.py, profiles/r29_wire_sets_rate.txt): N = 4 096 COMMIT messages of two
 * interleaved heights, V = 100, ten validators leave and ten join: one call 0.448 ms cold / 0.273 ms with known keys; per height
 * ibft_set_validators + ibft_verify_senders_wire 1.012 / 0.504 ms (0.44 x / 0.54 x; the host split not counted); ONE
 * ibft_verify_senders_wire over the batch, wrong for 200 rows, 0.417 / 0.240 ms (the price of the feature: + 0.03 ms).
 * Out of scope: ibft_verify_messages_wire and the certificate calls under a family, a streamed form and the group calls.
 * (Tallies per (height, round, type, hash): ibft_verify_senders_wire_views, below.)                                      */
#define IBFT_HEIGHT_RANGES_MAX 4096u
int ibft_set_height_sets(ibft_ctx *ctx, size_t n_ranges, const uint64_t *first_height, const uint32_t *range_set);
int ibft_height_sets_info(ibft_ctx *ctx, uint32_t *n_ranges, uint64_t *lo, uint64_t *hi);
int ibft_verify_senders_wire_sets(ibft_ctx *ctx, const uint8_t *wire, const uint32_t *off, size_t n, uint64_t *out_mask,
                                  ibft_wire_row_t *out_rows, int32_t *out_set, int32_t *out_vidx, ibft_tally_t *out_tally);

/* ---- the sets call plus ONE QUORUM RECORD per (height, round, type, proposal hash) of the batch -------------------------
 * The tallies of ibft_verify_senders_wire_sets are per SET; the reference asks per view and hash.  It keeps messages in
 * messages.Messages keyed by type, height, round and sender — a sender's later message REPLACES the earlier one
 * (messages/messages.go:64) — and asks HasQuorum / HasPrepareQuorum over GetValidMessages(view, type, isValid) on every
 * arriving message (core/ibft.go:1113-1121), in handlePrepare (:855-873, isValid = "names my proposal's hash") and in
 * handleCommit (:931-946).  ibft_verify_senders_wire_views answers that for every view and hash of a receive-queue batch
 * in the same call, on the device, and tells which rows a Messages store fed the batch in row order would still hold.
 *
 * out_mask, out_rows, out_set, out_vidx, out_tally: byte for byte what ibft_verify_senders_wire_sets returns for the same
 *   batch (its kernels run unchanged, in its order; the new work follows on the same stream before the one wait).
 * Definitions: a row is VALID when its final verdict bit is 1 (a member of its height's set, out_vidx >= 0); only PREPARE
 *   and COMMIT rows can be.  A valid row's VIEW is (height, round, type) of its parsed row, its KEY the view plus
 *   (hash_len, proposal_hash[0 .. hash_len)).
 * out_stored (a bit per row, ceil(n / 64) words; bits past n are 0): bit i is set iff row i is valid and no valid row
 *   j > i has the same view and the same sender (out_vidx under the same set) — the messages the store holds after
 *   AddMessage of every valid row in row order.  Per VIEW, not per key: a later message with another hash replaces too.
 * Views: the keys ordered by their lowest valid row, ascending; view v is the v-th key.  *out_n_views is the number of
 *   distinct keys and may exceed views_cap.  out_view[i] (n entries) is -1 for a row that is not valid, v for a valid row
 *   of view v < views_cap, -2 for a valid row whose view did not fit; -2 rows still supersede earlier rows of their
 *   sender in out_stored.  A views_cap above n behaves as n.
 * out_views: min(*out_n_views, views_cap, n) records, one per view (the caller provides min(views_cap, n) entries):
 *   height, round, type, hash_len, proposal_hash (bytes past hash_len zero) of the view's first row; set — the set of that
 *   height; first_row; rows — the valid rows with out_view == v; stored_rows — those of them with the stored bit;
 *   prepare_rule; tally.
 * Defining property of tally: with S_v the From column of the rows with out_view == v and the stored bit, in row order, it
 *   is field for field what ibft_set_validators(set) followed by ibft_tally(S_v, all-ones mask) returns — u64 and u256
 *   families (low 128 bits of the power, exact has_quorum), cold and warm, IBFT_FLAG_WIRE_RECODE on and off.  For a
 *   PREPARE record whose height is the height of the proposer table (ibft_set_proposers) and whose round lies inside it,
 *   prepare_rule = 1 and tally is instead what ibft_tally_prepare(S_v, all-ones, table[round]) returns — HasPrepareQuorum
 *   (validator_manager.go:99-127): the proposer's seat joins, a stored row FROM the proposer voids has_quorum and is
 *   counted in proposer_rows.  Otherwise prepare_rule = 0 and the plain rule holds.  The proposalMessage == nil case stays
 *   with the caller, as everywhere else.  A COMMIT record answers "who sent a valid COMMIT naming this hash as their last
 *   word in this view" and does not look at committed seals: ibft_verify_messages_wire_views, below, does.
 * Every output is a pure function of the batch, the family, the map, the proposer table and views_cap: nothing depends on
 *   the order threads arrive in, on the size of the device's tables or on the context's hash salt.
 * Errors: those of ibft_verify_senders_wire_sets in its order; views_cap == 0 with n > 0 is IBFT_E_INVAL and is checked
 *   with the argument checks in front — after "NULL ctx / NULL off / NULL out_mask", before the offsets are looked at, so
 *   before IBFT_E_TOOBIG and IBFT_E_NOVALSET.  out_mask is required when n > 0; every other out pointer may be NULL.  A
 *   refused call writes nothing.  n = 0: *out_n_views = 0 and out_tally as the sets call fills it.  Side effects (no
 *   resident staged batch, ibft_wire_stats, key cache, pipelines, the height map dropped by a call that fails midway):
 *   those of the sets call.  No new ibft_version().
 * The device groups through two open-addressing tables of row numbers (at least 2 n slots each, sized in the call) under a
 *   per-context random salt; scratch is sized by n and views_cap.  IBFT_WIRE_VIEWS_SLOTS (environment, tests only) lowers
 *   the slot count, never below the smallest power of two above n.
 * MEASURED (tools/wire_views_rate.py, profiles/r30_wire_views_rate.txt): N = 4 096 PREPARE and COMMIT
 * messages of two interleaved heights, V = 100, ten validators changed: 0.579 ms cold / 0.415 ms with known keys for six
 * views, 0.584 / 0.425 ms for 2 006 views (one validator's 2 000 PREPAREs each in a round of its own); the sets call alone
 * 0.451 / 0.288 ms (the records: + 0.13 ms); rows read back, grouped on the host, ibft_set_validators per height and
 * ibft_tally per record: 9.5 ms for six views (8.7 ms of it the tool's host pass in Python), 69 ms for 2 006.
 * Out of scope: a streamed form, a group form.  (The COMMIT seals of a record's rows: ibft_verify_messages_wire_views.)  */
typedef struct {
  uint64_t height, round; /* the view's                                                             */
  int32_t set;            /* the set of the family the view's height is judged under                */
  uint32_t first_row;     /* the lowest valid row of the key                                        */
  uint32_t rows;          /* valid rows with out_view == v                                          */
  uint32_t stored_rows;   /* ... of them with the stored bit: the length of S_v                     */
  uint8_t type;           /* IbftMessage.type: 1 PREPARE, 2 COMMIT                                  */
  uint8_t hash_len;       /* proposal hash bytes present (<= 32)                                    */
  uint8_t prepare_rule;   /* 1: tally follows HasPrepareQuorum with the table's proposer            */
  uint8_t pad[5];
  uint8_t proposal_hash[32];
  ibft_tally_t tally;
} ibft_wire_view_t; /* 128 bytes */
int ibft_verify_senders_wire_views(ibft_ctx *ctx, const uint8_t *wire, const uint32_t *off, size_t n, size_t views_cap,
                                   uint64_t *out_mask, ibft_wire_row_t *out_rows, int32_t *out_set, int32_t *out_vidx,
                                   ibft_tally_t *out_tally, int32_t *out_view, uint64_t *out_stored,
                                   ibft_wire_view_t *out_views, uint32_t *out_n_views);

/* ---- the views call with the COMMITTED SEALS checked inside the COMMIT records ------------------------------------------
 * handleCommit (core/ibft.go:931-946) counts a stored COMMIT only if IsValidCommittedSeal(proposalHash, seal) holds; a COMMIT
 * record of ibft_verify_senders_wire_views counts every stored COMMIT with a valid envelope, whatever its seal — an upper
 * bound.  This call judges the seals in the SAME verdict launch as the envelopes (sender rows [0, n), the sealable rows'
 * seals dense behind them from ceil(n / 64) * 64 on, the tail pre-flagged) and tallies a COMMIT record over stored AND
 * sealed.
 *
 * out_mask, out_rows, out_set, out_vidx, out_tally, out_view, out_stored, *out_n_views: byte for byte what
 *   ibft_verify_senders_wire_views returns for the same batch; so is every field of out_views but pad[0] and tally of COMMIT
 *   records.  PREPARE records are the views call's, byte for byte.
 * A row is SEALABLE when its status is OK, it has a set (out_set >= 0), type == 2 with a CommitMessage payload, a 20-byte
 *   From, a 65-byte seal and a 32-byte proposal hash, and its From is a member of the row's set — a table lookup in front of
 *   the verdict launch: an outsider, or a member of the union outside the row's set, loses its sender bit whatever its
 *   signature says and buys no second ECDSA.  A hash that is not 32 bytes equals no proposal hash: no arithmetic either.
 * out_seal (a bit per row, ceil(n / 64) words; bits past n are 0; may be NULL): bit i is set iff row i is valid AND
 *   sealable AND its seal recovers to its From over the digest the context's seal-digest convention (ibft_set_seal_digest)
 *   derives from the carried hash.  Defining property: for every set s the seal bits of the valid COMMIT rows with
 *   out_set == s, in row order, are bit for bit what ibft_set_validators(set s) followed by ibft_verify_seals(proposal_hash,
 *   seal, From) over those rows returns, a row that is not sealable pre-flagged — under IBFT_SEAL_DIGEST_IDENTITY and
 *   _KECCAK_SUFFIX, cold and warm, u64 and u256 powers, IBFT_FLAG_WIRE_RECODE on and off (a recoded row's seal is the one
 *   the recode walk stored).  The bit is defined for every valid COMMIT row, stored or not.
 * A COMMIT record (type == 2) has pad[IBFT_WIRE_VIEW_SEAL_RULE] = 1 and its tally is field for field what
 *   ibft_set_validators(set) followed by ibft_tally(S_v, mask = the seal bits of S_v) returns, S_v as in the views call:
 *   rows and stored_rows keep their meaning, tally.valid_rows <= stored_rows.  The stored rule stays per view: a sender
 *   whose stored (latest) COMMIT of the view has a bad seal contributes nothing, even if a superseded row of theirs had a
 *   good one — the store holds one message per sender and GetValidMessages filters it.  The COMMIT record of the accepted
 *   proposal's hash is handleCommit's hasQuorumByMsgType; the seals for setCommittedSeals are the rows with out_view == v,
 *   the stored bit and the seal bit.
 * Errors, side effects, optional pointers: exactly those of ibft_verify_senders_wire_views, in its order; a refused call
 *   writes nothing.  The first call grows the context's row columns to twice max_rows (as ibft_verify_messages_wire does);
 *   contexts that never make it allocate nothing more.  The two views calls may alternate on one context.
 * ibft_wire_seal_stats: two counts of the last ibft_verify_messages_wire_views of the context — commit_rows, the COMMIT
 *   rows (status OK, type 2, CommitMessage) that have a set; seal_rows, the sealable rows, i.e. the seal checks the verdict
 *   launch was given.  0 / 0 after any other wire call.  IBFT_E_INVAL for a NULL ctx; either pointer may be NULL.
 * MEASURED (tools/wire_view_seals_rate.py, profiles/r31_wire_view_seals_rate.txt; kernels:
 * profiles/r31_kernel_meta_wire_view_seals.txt): the batch of the views call's measurement, N = 4 096 messages of two
 * interleaved heights, V = 100, every seal valid; median of 25 single calls.  All COMMITs (4 096 seal rows): 0.960 ms cold /
 * 0.545 ms with known keys against 0.605 / 0.430 ms for the views call alone: the seals cost + 0.355 / + 0.115 ms, where ONE
 * ibft_verify_seals over the same 4 096 rows takes 0.363 / 0.182 ms.  PREPAREs and COMMITs half and half (2 000 seal rows):
 * 0.908 / 0.501 ms against 0.567 / 0.389 ms (+ 0.341 / + 0.112 ms; one ibft_verify_seals of the 2 000: 0.442 / 0.169 ms).
 * What a caller of the views call does for the same answer — rows read back, the 200 STORED COMMIT rows gathered per height,
 * ibft_set_validators + ibft_verify_seals per height, ibft_tally per COMMIT record — takes 1.300 / 0.906 ms and 1.257 /
 * 0.857 ms, of it 0.02 - 0.03 ms the host gather (numpy index selections over a seal column prepared beforehand); that route
 * checks 200 seals where this call checks every valid COMMIT's.  The views call itself reads 0.595 and 0.608 ms cold, 0.406 and
 * 0.445 ms warm on this build against 0.598 and 0.612, 0.432 and 0.435 ms on the parent's library in the same lease.
 * Out of scope: streamed and group forms.  No new ibft_version().                                                       */
#define IBFT_WIRE_VIEW_SEAL_RULE 0 /* index into ibft_wire_view_t.pad: 1 = the record's tally counts only rows whose committed seal verifies */
int ibft_verify_messages_wire_views(ibft_ctx *ctx, const uint8_t *wire, const uint32_t *off, size_t n, size_t views_cap,
                                    uint64_t *out_mask, ibft_wire_row_t *out_rows, int32_t *out_set, int32_t *out_vidx,
                                    ibft_tally_t *out_tally, int32_t *out_view, uint64_t *out_stored,
                                    ibft_wire_view_t *out_views, uint32_t *out_n_views, uint64_t *out_seal);
int ibft_wire_seal_stats(ibft_ctx *ctx, uint32_t *commit_rows, uint32_t *seal_rows);

/* a8 alone: HasQuorum over the rows whose bit is set in mask.                      */
int ibft_tally(ibft_ctx *ctx, const uint8_t *sender20, const uint64_t *mask, size_t n,
               ibft_tally_t *tally);
/* a8, the PREPARE form: ValidatorManager.HasPrepareQuorum(state, proposalMessage, msgs)
 * (/root/reference/core/validator_manager.go:99-127 — what hasQuorumByMsgType asks for PREPARE messages,
 * core/ibft.go:1273-1284).  proposer20 = proposalMessage.From.  The proposer's address JOINS the sender set before the
 * powers are summed (it counts once, and only if it is a validator: unknown addresses add nothing, :88-92), and a
 * row of the mask whose sender equals the proposer byte for byte — validator or not — voids the result:
 * has_quorum = 0 whatever the power, tally->proposer_rows = the number of such rows (:114-121 "proposer is among
 * signers but it is not expected to be").  distinct_senders then counts the proposer's seat too.  With n = 0 the
 * answer is whether the proposer alone is a quorum (one validator of all the power).  The caller keeps the one case
 * the device cannot see: proposalMessage == nil → false without asking (:101-110).  The same rule is applied by
 * ibft_verify_messages / ibft_verify_messages_wire / ibft_group_verify_messages when their proposer20 argument is
 * not NULL, and by the sharded merge (the seat joins the MERGED bitmap; a proposer row in any shard voids).     */
int ibft_tally_prepare(ibft_ctx *ctx, const uint8_t *sender20, const uint64_t *mask, size_t n,
                       const uint8_t proposer20[20], ibft_tally_t *tally);

/* The context remembers the last (raw proposal, round) it hashed: ibft_verify_hashes / ibft_verify_messages
 * with the same proposal do not hash it again.  ibft_forget_proposal drops that memory (the next call hashes);
 * bench.py calls it once per measured sequence so that every height pays for its own proposal hash.         */
int ibft_forget_proposal(ibft_ctx *ctx);

/* ---- staged (device-resident) form of a2, used by bench.py and by multi-GPU ----
 * stage:  copy the batch into the context's HBM columns (H2D, synchronous).
 * launch: enqueue unpack → recover → tally on the context's stream (asynchronous);
 *         `repeat` back-to-back passes over the resident batch (each pass is the
 *         full computation; used to time K steps without host round trips).
 * fetch:  wait for the stream, copy mask + tally back.                             */
int ibft_seals_stage(ibft_ctx *ctx, const uint8_t *hash32, const uint8_t *sig65,
                     const uint8_t *signer20, const uint8_t *pre_flags, size_t n);
int ibft_seals_launch(ibft_ctx *ctx, uint32_t repeat);
int ibft_seals_fetch(ibft_ctx *ctx, uint64_t *out_mask, ibft_tally_t *tally);
/* launch(1) + fetch in one call: one more pass over the resident batch, results on return.      */
int ibft_seals_run(ibft_ctx *ctx, uint64_t *out_mask, ibft_tally_t *tally);
/* Two staging slots (round 5): the reference hands handleCommit NEW messages at every wake-up
 * (core/ibft.go:931-946: one GetValidMessages walk per wake-up), so a sustained stream of batches pays an upload per
 * batch; with one column set the upload of batch k+1 could not start before the verdict of batch k.
 *   ibft_seals_stage_next: copy the NEXT batch into the context's spare column set on a copy stream of its own,
 *       asynchronously — the source buffers must stay untouched until ibft_seals_swap(ctx, 1) returns (or, with
 *       wait_for_copy = 0, until the next fetch of that batch); for the copy to overlap they must be page-locked
 *       (ibft_pinned_alloc);
 *   ibft_seals_swap: the staged batch becomes the resident one (launch / run / fetch then work on it), the previous one
 *       becomes the spare slot; kernels already enqueued keep reading the columns they were launched on, the ones
 *       enqueued afterwards wait ON THE DEVICE for the copy.  IBFT_E_INVAL without a staged batch.
 * Per step of a sustained stream:  launch(k) → stage_next(k+1) → fetch(k) → swap.                                   */
/* Pipelined passes (round 5): ibft_seals_submit enqueues ONE pass over the resident batch (verdict kernel + tally) whose
 * results go to one of two host-visible result slots, and returns at once; ibft_seals_collect waits for the OLDEST
 * submitted pass — the event behind its tally, not the whole stream — and delivers its verdict words and tally.  At most
 * two passes in flight (IBFT_E_INVAL beyond; IBFT_E_INVAL on a collect with nothing submitted).  With one pass kept in
 * flight the launch of pass k+1 overlaps the completion, result delivery and host handling of pass k: the device runs
 * back to back, as a node's does when batches arrive faster than one host round trip (and as a rank's does in the
 * sharded form, where exchange k overlaps the kernels of pass k+1).  Combines with the staging slots:
 * submit(k) → stage_next(k+1) → collect(k−1) → swap.
 * out_mask of a collect holds ⌈rows/64⌉ words for the rows of THAT pass (the batch resident when it was submitted —
 * ibft_seals_rows says how many; a swap in between may have changed the resident batch's size).  With the key cache on, a
 * collect whose pass taught the device new keys builds their tables before it returns, which drains the context's whole
 * stream — the newer pass in flight included: the cold-to-warm transition costs one full wait.  A failure of that table
 * build takes nothing from the pass just delivered (IBFT_OK, verdicts valid); the next ibft_seals_submit returns it.   */
int ibft_seals_submit(ibft_ctx *ctx);
int ibft_seals_collect(ibft_ctx *ctx, uint64_t *out_mask, ibft_tally_t *tally);
/* Rows of the resident seal batch, and of the oldest pass submitted and not yet collected (0: none in flight): what a
 * binding sizes the out_mask of ibft_seals_run / _fetch / _collect from.                                              */
int ibft_seals_rows(ibft_ctx *ctx, uint32_t *resident_rows, uint32_t *oldest_pass_rows);
/* Round 6: the TALLY of a submitted pass (HasQuorum over the rows that passed, core/validator_manager.go:77-96) runs on a
 * stream of its own, next to the verdict kernel of the pass submitted after it, on a second copy of the work buffers the
 * two would share — the device goes from verdict kernel to verdict kernel without the tally and its two dependency gaps in
 * between (9–15 µs per pass).  Same results, slot for slot; every other entry point first puts the context's main stream
 * behind the tallies still in flight.  Not for a rank of a sharded batch (its exchange follows the tally) and not while
 * the key cache is still learning.  IBFT_SIDE_TALLY=0 keeps everything on one stream (A/B).
 * ibft_pipeline_stats: passes whose tally took the side stream, and batches of 65 537 … 98 304 rows that went out as two
 * launches (both since the context was created; either pointer may be NULL).                                             */
int ibft_pipeline_stats(ibft_ctx *ctx, uint32_t *side_tallies, uint32_t *split_batches);
/* Round 21: consecutive submitted passes may put their VERDICT launch alternately on the context's main stream and on a
 * second stream, so that pass k+1 starts in the tail of pass k (whose helper wavefronts have left their registers) instead
 * of behind it.  Same results, slot for slot; applies only where the side-stream tally applies, and by default only to the
 * kernel forms it was measured to pay for.  IBFT_ALT_VERDICT=0 keeps every verdict launch on the main
 * stream, =1 alternates wherever the conditions hold (A/B, tests).  Every other entry point is behind both streams.
 * ibft_pipeline_stats_ex: ibft_pipeline_stats plus the passes whose verdict launch took the second stream (any pointer may
 * be NULL).  No new ibft_version(): a build without the symbol simply lacks it.                                          */
int ibft_pipeline_stats_ex(ibft_ctx *ctx, uint32_t *side_tallies, uint32_t *split_batches, uint32_t *alt_verdicts);
int ibft_seals_stage_next(ibft_ctx *ctx, const uint8_t *hash32, const uint8_t *sig65,
                          const uint8_t *signer20, const uint8_t *pre_flags, size_t n);
int ibft_seals_swap(ibft_ctx *ctx, int wait_for_copy);
/* Device address of the resident verdict mask (⌈n/64⌉ u64 words) and of the two
 * u64 tally accumulators {power, valid_rows|distinct<<32}: lets the caller run an
 * RCCL all-reduce over validator shards without a host round trip.                 */
int ibft_seals_device_ptrs(ibft_ctx *ctx, void **d_mask, size_t *mask_words, void **d_tally);
/* Copy the resident verdict mask (⌈n/64⌉ u64) and the 4 tally words {power_lo,
 * power_hi, valid_rows|distinct<<32, has_quorum} into caller-owned DEVICE buffers
 * (e.g. a torch tensor's data_ptr) and wait for the copy: the hand-off point to an
 * RCCL all-reduce issued by the caller.  Either pointer may be NULL.               */
int ibft_seals_export(ibft_ctx *ctx, void *d_mask_dst, void *d_tally_dst);
/* Same hand-off without a host round trip: the copies are enqueued on the CALLER's stream (a
 * hipStream_t, e.g. torch.cuda.current_stream().cuda_stream — the one the collective will run on)
 * behind an event that marks the last launch's results ready, and the context's next tally waits
 * (on the device) until they have been read.  The caller's collective then overlaps with the next
 * ibft_seals_launch on the context's own stream.                                                  */
int ibft_seals_export_on(ibft_ctx *ctx, void *d_mask_dst, void *d_tally_dst, void *consumer_stream);
/* HIP-event time (ms) of the verdict kernels, measured on the context's own stream, summed over the
 * launches since the previous call of this function (which resets the sum), and their count.      */
int ibft_last_kernel_ms(ibft_ctx *ctx, float *ms, uint32_t *launches);
/* Time the verdict kernels of every n-th staged pass only (default 1 = every pass, 0 = never): an event pair
 * costs ≈5 µs of a 0.45 ms step (profiles/r02_launch_gap.txt).                                            */
int ibft_set_kernel_timing(ibft_ctx *ctx, uint32_t every_n);
/* Warm-path statistics: validators whose table is built, how many verdict passes ran with /
 * without the warm kernel since the context was created, and the lanes-per-signature (64 = one
 * wavefront per signature … 1 = lane kernel) the last warm pass used.                         */
int ibft_cache_stats(ibft_ctx *ctx, uint32_t *tables, uint32_t *warm_passes, uint32_t *cold_passes,
                     uint32_t *lanes_per_signature);
/* The key tables belong to the DEVICE: every context created on one device shares ONE fixed-base table of G (84 MB) and ONE
 * pool of validator tables keyed by ADDRESS (655 KB per validator, IBFT_QTAB_BUDGET_GB, default 64) — the four contexts a
 * Backend keeps for its four goroutines cost one pool, not four; a key learned through one context is
 * known to all of them; a validator that stays in the set across ibft_set_validators keeps its table (a rotation of 1 % of
 * the validators relearns 1 %), a slot nobody's current set refers to is reused (its state reads "unknown" again before any
 * kernel can see it: the old key and table left in it are never consulted).  The pool never holds more than
 * IBFT_QTAB_BUDGET_GB / 655 360 slots: validators of a set beyond that have no slot and are served by the recover path for
 * good (verdicts unchanged; ibft_cache_stats never reports every table built for such a set), and a budget of 0 turns the
 * cache off without an error.  This reports the shared object of ctx's device: bytes it holds, slots in use / allocated, and
 * how many contexts share it (tests/test_gpu_key_cache_lifecycle.py pins all of this in fresh processes).
 *
 * THE TABLE FORM belongs to the pool, so it is the device's and not a context's: the environment variable
 * IBFT_QTAB_FORM=wide|glv is read when the FIRST context of a device is created (the device's shared object lives as long as
 * one context of the device does); unset means wide; any other value makes that ibft_ctx_create fail with IBFT_E_INVAL, and
 * ibft_last_error(NULL), asked on the same thread, names the variable.  wide: 32 windows × 256 points over u2, 655 360 B per validator.  glv: u2 is split
 * with the curve's endomorphism and recoded in signed digits, 16 windows (15 × 128 points and one of 256) serve both halves,
 * 174 080 B per validator — 3.76 times as many slots per IBFT_QTAB_BUDGET_GB (6 168 instead of 1 638 per GiB), the pool, its
 * growth and ibft_cache_memory's bytes scale with it, and a table build writes that much less.  What the form does NOT change:
 * every verdict, tally and error code of every entry point, the slot state machine, which kernel width a batch gets
 * (ibft_last_dispatch), the 84 MB table of G; a signature sums 48 table points in both.                               */
int ibft_cache_memory(ibft_ctx *ctx, uint64_t *device_bytes, uint32_t *slots_in_use, uint32_t *slots_allocated,
                      uint32_t *contexts_sharing);
/* The pool's table form: 0 = wide, 1 = glv, and the bytes of one slot's table (655 360 / 174 080).  Any out pointer may be NULL;
 * IBFT_E_INVAL for a NULL ctx.                                                                                           */
int ibft_cache_form(ibft_ctx *ctx, uint32_t *form, uint64_t *slot_bytes);
/* Lanes per signature used by the last verdict pass: cold kernel (1 = ecrecover_lane_kernel,
 * 2/4/8 = ecrecover_group_kernel, 16 = ecrecover_rows_kernel, 64 = ecrecover_wave_kernel, 128 = ecrecover_wave2_kernel)
 * and warm kernel (0 = none ran, 1 = lane, 2..64 = group).                                        */
int ibft_last_dispatch(ibft_ctx *ctx, uint32_t *cold_lanes, uint32_t *warm_lanes);
/* (A cold batch of 65 537 … 98 304 rows is two launches — 65 536 rows through the lane kernel with its tables in LDS, the rest
 * through the kernel the rule above picks for that many rows — and reports cold_lanes = 1, table 1; IBFT_SPLIT_LARGE=0 in the
 * environment pins one launch of the private-segment lane kernel.)                                                        */
/* Where the last lane / group cold kernel kept the per-lane window table of u2·R: 0 = no such kernel ran, 1 = the
 * workgroup's LDS (default up to one wavefront per SIMD: no private segment), 2 = private segment with the entries read in
 * front of the doublings (round 4's form; IBFT_COLD_TABLE=private), 3 = private segment without that prefetch — two
 * resident wavefronts per SIMD, the lane kernel's form beyond 65 536 rows.                                              */
int ibft_last_cold_table(ibft_ctx *ctx, uint32_t *table);
/* ---- pinned column buffers -------------------------------------------------------------------------
 * Every entry point accepts ordinary (pageable) host memory for its columns; the runtime then stages each
 * column through its own bounce buffer — measured at ≈8.5 GB/s, 0.15 ms for the 1.3 MB of a 4 096-message
 * COMMIT set (profiles/r02g_seq_*).  A caller that flattens messages into columns anyway (the cgo shim's
 * SoA batcher) should write them into buffers from ibft_pinned_alloc instead: page-locked
 * memory the device reads directly — when every column of a call lies in such buffers the library replaces
 * the per-column copy commands by ONE gather launch (≈8 µs of host time per column saved, the copies no
 * longer queue one behind the other).  Plain memory otherwise: valid until ibft_pinned_free, usable with
 * any context, any thread.  Returns NULL when the runtime refuses (no device, out of lockable memory).     */
void *ibft_pinned_alloc(size_t bytes);
void ibft_pinned_free(void *p);
/* Batches of this context whose columns ALL lay in ibft_pinned_alloc blocks and were therefore read by the
 * device in one gather launch instead of one copy command per column (environment IBFT_NO_GATHER=1 turns
 * the gather off: pinned columns then take the copy commands, still faster to issue than pageable ones).  */
int ibft_column_stats(ibft_ctx *ctx, uint32_t *gather_batches);

/* ---- a whole PREPARE / COMMIT set in one call --------------------------------------------------------
 * The reference judges a stored PREPARE / COMMIT message three times, at different moments: IsValidValidator
 * when it arrives (core/ibft.go:1128, core/backend.go:41-45), IsValidProposalHash and — COMMIT only —
 * IsValidCommittedSeal when the view is handled (core/ibft.go:856-862 handlePrepare's closure, :932-944
 * handleCommit's).  All three are pure functions of the message bytes, the proposal and the validator set, so
 * a Backend that receives messages in batches can have the whole set judged at once:
 *   out_sender_mask bit i = IsValidValidator(message i)            — what AddMessage would have decided;
 *   out_valid_mask  bit i = hash32[i] ≡ keccak(raw ‖ BE64(round))  (hash_len[i] == 32)
 *                           ∧ (seal65 == NULL ∨ IsValidCommittedSeal(hash32[i], {from20[i], seal65[i]}))
 *                         — what the handle* closure would return for it;
 *   tally                 = ValidatorManager.HasQuorum over the rows with both bits (hasQuorumByMsgType of
 *                           the messages that were stored AND survive the closure); with proposer20 != NULL
 *                           (a PREPARE set: proposer20 = the accepted proposal message's From) the tally is
 *                           ValidatorManager.HasPrepareQuorum — see ibft_tally_prepare.
 * payload / off / msg_sig65 / from20 / sender_pre are ibft_verify_senders' columns (sender_pre = its pre_flags),
 * hash32 / hash_len are ibft_verify_hashes', seal65 / valid_pre are ibft_verify_seals' sig65 / pre_flags
 * (seal65 NULL for a PREPARE set; the seal's signer is the message's From, messages/helpers.go:22-35).  The proposal is given as raw bytes + round (hashed on the
 * device once and remembered, like ibft_verify_hashes) or, when digest32 != NULL, as its 32-byte digest.
 * sender_pre[i] != 0 clears the sender bit of row i, valid_pre[i] != 0 its valid bit (either may be NULL).
 * Both signatures of every message go through ONE verdict
 * launch of 2n rows: at n = 4 096 that is two wavefronts per SIMD instead of one, 0.70 ms for 8 192
 * signatures against 2 × 0.45 ms (profiles/).  Verdicts are bit-identical to the three separate calls.     */
int ibft_verify_messages(ibft_ctx *ctx, const uint8_t *payload, const uint32_t *off, const uint8_t *msg_sig65,
                         const uint8_t *from20, const uint8_t *hash32, const uint8_t *hash_len,
                         const uint8_t *seal65, const uint8_t *sender_pre, const uint8_t *valid_pre, size_t n,
                         const uint8_t *raw, size_t raw_len, uint64_t round, const uint8_t *digest32,
                         const uint8_t *proposer20, uint64_t *out_sender_mask, uint64_t *out_valid_mask,
                         ibft_tally_t *tally);

/* The same for a batch of messages AS THE TRANSPORT DELIVERED THEM (ibft_verify_senders_wire's input): the
 * device walks the bytes, and every canonical PREPARE / COMMIT message of the view (height, round) is judged
 * completely in one verdict launch — no proto.Unmarshal, no PayloadNoSig re-marshal, no flattening on the host.
 *   out_sender_mask bit i = IsValidValidator(message i)        (0 for rows with out_rows[i].status ==
 *                           IBFT_WIRE_NEEDS_HOST: those take the stock route, exactly as after
 *                           ibft_verify_senders_wire);
 *   out_valid_mask  bit i = message i is a PREPARE or COMMIT of (height, round) — type and payload agree, 20-byte
 *                           From, 65-byte seal for a COMMIT — whose 32-byte proposal hash equals the proposal's
 *                           and, for a COMMIT, whose committed seal verifies for From: the handlePrepare /
 *                           handleCommit closure (core/ibft.go:856-862, :932-944).  Messages of other views or
 *                           kinds have bit 0 here and are judged when their view is handled;
 *   tally                 = HasQuorum over the rows with both bits (meaningful for a batch of one type) —
 *                           HasPrepareQuorum when proposer20 != NULL (a batch of PREPAREs of the asked view; in a
 *                           batch of both types only a PREPARE of the proposer counts in proposer_rows and voids
 *                           the quorum — his COMMIT is no PREPARE of his, validator_manager.go:114-121);
 *   out_class[i] (n bytes, may be NULL) = what the caller needs to route row i: IBFT_WIRE_CLASS_NEEDS_HOST — not
 *                           judged here, stock route; IBFT_WIRE_CLASS_CLOSURE — a PREPARE / COMMIT of the asked
 *                           view: its valid bit IS the closure's verdict; bits 4..7 = IbftMessage.type.  One byte
 *                           per row, delivered with the masks;
 *   out_rows (may be NULL) = the full parse results, 80 B per row through a copy command — only when the
 *                           fields themselves are wanted.
 * The proposal: raw + proposal_round (hashed once and remembered) or digest32, as in ibft_verify_messages.   */
#define IBFT_WIRE_CLASS_NEEDS_HOST 0x01u
#define IBFT_WIRE_CLASS_CLOSURE 0x02u
int ibft_verify_messages_wire(ibft_ctx *ctx, const uint8_t *wire_bytes, const uint32_t *off, size_t n,
                              uint64_t height, uint64_t round, const uint8_t *raw, size_t raw_len,
                              uint64_t proposal_round, const uint8_t *digest32, uint64_t *out_sender_mask,
                              uint64_t *out_valid_mask, uint8_t *out_class, ibft_wire_row_t *out_rows,
                              const uint8_t *proposer20, ibft_tally_t *tally);

/* ---- SURVEY.md §8f rank 2 from the transport's bytes: certificates --------------------------------------------
 * A PREPREPARE message carries a RoundChangeCertificate, a ROUND_CHANGE message a PreparedCertificate
 * (/root/reference/messages/proto/messages.proto:46-57, 73-101): IbftMessages inside IbftMessages.  The reference
 * verifies every one of them — validateProposal / validPC / handleRoundChangeMessage → GetExtendedRCC
 * (/root/reference/core/ibft.go:470-551, 683-788, 1162-1231; messages/messages.go:202-245): IsValidValidator on the
 * envelope of each nested message (PayloadNoSig re-marshalled per message, proto/helper.go:12-27) and
 * IsValidProposalHash on the hash each one carries — O(N²) signatures per round change, after proto.Unmarshal has
 * materialised the whole pointer graph.  This call takes the messages AS THE TRANSPORT DELIVERED THEM (row i of the call
 * is wire[off[i]..off[i+1]), any IbftMessage type) and judges the whole tree on the device:
 *
 *   rows      one per IbftMessage of the tree, breadth first: rows [0, n) are the call's messages (level 0), the
 *             messages nested directly inside level-k rows are level k + 1 — children of row i before children of row
 *             j > i, a row's children in wire order (PreparedCertificate: proposalMessage first, then prepareMessages;
 *             RoundChangeCertificate: roundChangeMessages).  *out_n_rows = their number.  Because a decoded message
 *             lists its nested messages in the same order, the host maps row → *proto.IbftMessage by position.
 *   out_nodes[row]  where the row lies and what it is to its parent (ibft_cert_node_t), may be NULL
 *   out_rows[row]   its parsed fields, as ibft_verify_senders_wire reports them; payload_kind 5 / 8 rows carry
 *                   PrePrepareMessage.proposalHash in proposal_hash.  May be NULL
 *   out_class[row]  0 = judged here.  IBFT_CERT_CLASS_NEEDS_HOST: the bytes of this message — or of a message below it —
 *                   are not the canonical encoding (unknown fields, non-minimal varints, …): PayloadNoSig is not
 *                   "bytes minus the signature field", the sender bit is 0 and the caller decides this message by the stock
 *                   route (rows below it that are canonical are still judged).  IBFT_CERT_CLASS_DIGEST_BY_HOST: canonical
 *                   but longer than IBFT_CERT_DIGEST_MAX_BYTES — Keccak is sequential: the wavefront that hashes a long
 *                   message absorbs ≈25 MB/s — so the sender bit is 0 and the host hashes bytes[0, cut0) ‖ bytes[cut1, len)
 *                   itself (out_nodes) and asks ibft_verify_seals with that digest.  IBFT_CERT_CLASS_PROPOSAL_BY_HOST: the Proposal this message
 *                   carries is that long: the self bit of this row and the hash bits of its children are undecided
 *   out_sender_mask bit row = IsValidValidator(message): its envelope signature recovers to From, From is a validator
 *   out_hash_mask   bit row = the 32-byte proposal hash this message carries equals keccak(lastPreparedProposal) of the
 *                   ROUND_CHANGE message whose PreparedCertificate contains it (proposalMatchesCertificate,
 *                   core/ibft.go:516-551: IsValidProposalHash(proposal, hash) for every message of the certificate); 0 for
 *                   rows that are not inside a PreparedCertificate
 *   out_self_mask   bit row = a PREPREPARE payload's proposalHash equals keccak(its own Proposal)
 *                   (validateProposalCommon, core/ibft.go:640-651)
 * All masks have room for ⌈rows_cap/64⌉ words (the first ⌈*out_n_rows/64⌉ are written); out_hash_mask, out_self_mask and out_class may
 * be NULL.  The tree must fit rows_cap and the context's max_rows: IBFT_E_TOOBIG otherwise
 * (no verdicts — split the call or take the stock route).  What stays with the caller is everything that is not
 * arithmetic: types, views, rounds, proposer and quorum rules over the From / type / view columns.               */
#define IBFT_CERT_CLASS_NEEDS_HOST 0x01u
#define IBFT_CERT_CLASS_DIGEST_BY_HOST 0x02u
#define IBFT_CERT_CLASS_PROPOSAL_BY_HOST 0x04u
#define IBFT_CERT_DIGEST_MAX_BYTES (1u << 20)
#define IBFT_CERT_ROLE_ROOT 0u          /* one of the call's n messages                          */
#define IBFT_CERT_ROLE_PC_PROPOSAL 1u   /* PreparedCertificate.proposalMessage                   */
#define IBFT_CERT_ROLE_PC_PREPARE 2u    /* PreparedCertificate.prepareMessages[k]                */
#define IBFT_CERT_ROLE_RCC_MESSAGE 3u   /* RoundChangeCertificate.roundChangeMessages[k]         */
#define IBFT_CERT_HAS_PROPOSAL 0x01u    /* flags: a Proposal sub-message is present              */
#define IBFT_CERT_HAS_CERTIFICATE 0x02u /* flags: a certificate wrapper is present               */
#define IBFT_CERT_NO_PARENT 0xFFFFFFFFu
typedef struct {
  uint32_t off, len;                /* the message's bytes in `wire`                                             */
  uint32_t parent, ordinal;         /* containing row (IBFT_CERT_NO_PARENT for level 0), position among its children */
  uint32_t first_child, n_children; /* its nested messages are rows [first_child, first_child + n_children);
                                       first_child means nothing when n_children == 0 (test n_children first)   */
  uint32_t raw_off, raw_len;        /* Proposal.rawProposal it carries (PREPREPARE: proposal; ROUND_CHANGE:
                                       lastPreparedProposal), in `wire`                                          */
  uint64_t proposal_round;          /* Proposal.round                                                            */
  uint32_t cut0, cut1;              /* its signature field (tag, length, bytes) relative to off                  */
  uint8_t level, role, flags;       /* IBFT_CERT_ROLE_*, IBFT_CERT_HAS_* (the class bits 0x04 / 0x08 mirror out_class) */
  uint8_t pad[5];
} ibft_cert_node_t;
int ibft_verify_certificates_wire(ibft_ctx *ctx, const uint8_t *wire, const uint32_t *off, size_t n, size_t rows_cap,
                                  size_t *out_n_rows, ibft_cert_node_t *out_nodes, ibft_wire_row_t *out_rows,
                                  uint8_t *out_class, uint64_t *out_sender_mask, uint64_t *out_hash_mask,
                                  uint64_t *out_self_mask);

/* ---- certificates judged per carrier -----------------------------------------------------------------------------
 * The same call, and on top of it what the reference asks PER CERTIFICATE, computed on the device: one fixed-size record
 * for every message that can carry a certificate the caller has to decide —
 *
 *   every level-0 row (the call's n messages), and
 *   every level-1 row of role IBFT_CERT_ROLE_RCC_MESSAGE (the ROUND_CHANGE messages in a root PREPREPARE's
 *   RoundChangeCertificate; deeper certificates — a PreparedCertificate's proposal message carrying an RCC of its own —
 *   get no record),
 *
 * in ascending row order (out_cert[i].row == i for i < n).  *out_n_certs = their number; more than certs_cap:
 * IBFT_E_TOOBIG.  A record holds
 *
 *   pc    validPC (core/ibft.go:1162-1231) with AreValidPCMessages / HasUniqueSenders (messages/helpers.go:148-213) for the
 *         PreparedCertificate of a ROUND_CHANGE row, everything but the proposer rule: −1 undecided here (an irregular shape —
 *         a nested message that is not judged, has no view, a From longer than 20 bytes, a payload that disagrees with its
 *         type, nested messages of its own …: decide it by the walk over the decoded message), 0 invalid, 1 valid up to
 *         IsProposer, 2 the message carries no certificate.  A root ROUND_CHANGE is judged against its own view (round limit =
 *         its round) and with proposalMatchesCertificate (:516-551: every hash bit of the certificate); a ROUND_CHANGE inside a
 *         root PREPREPARE's certificate against the PREPREPARE's height and round, without (validateProposal, :746-778).
 *         When pc == 1: pc_round, pc_from, pc_hash = view round, From and carried hash of the certificate's proposal message.
 *   rcc   a root PREPREPARE's RoundChangeCertificate (validateProposal, :697-778): unique senders, their quorum, every message
 *         a validly signed ROUND_CHANGE of the PREPREPARE's view, every prepared certificate below decided: −1 / 0 / 1 / 2 as
 *         above (−1 too when a child's pc is −1); rcc_rows = the rows of the certificate's subtree down to level 2 (meaningful
 *         for rcc ≥ 0).  −1 for every other record.
 *   first_child_cert  for a root PREPREPARE with a RoundChangeCertificate: out_cert[first_child_cert + k] is the record of its
 *         k-th nested message (k < n_children); IBFT_CERT_NO_RECORD otherwise.
 *   row, first_child, n_children, cls, the row's own type / role / level / height / round / from, and in bits its own sender,
 *   hash and self bit with IBFT_CERT_HAS_PROPOSAL / _CERTIFICATE of its node.
 *
 * How a caller finishes:
 *   validPC(latestPC, limit, height)   pc == 2: true.  pc == 1: IsProposer(pc_from, height, pc_round).  0: false.
 *   handleRoundChangeMessage's closure (:478-489)   the same, and for pc == 2: the message must carry no proposal either
 *         (bits & IBFT_CERT_BIT_HAS_PROPOSAL → false).
 *   validateProposal's certificate half   rcc == 1: walk the records of the certificate; among those whose validPC holds the
 *         highest pc_round wins, the LAST one among equals: (pc_round, pc_hash) is the prepared proposal's — O(Q), no row read.
 * THE CONTRACT this rests on: IsProposer accepts at most one address per (height, round).  validPC also demands that no PREPARE
 * of the certificate comes from the proposer; with unique senders (part of pc == 1) and a proposal message from THE proposer no
 * other message can.  A Backend whose IsProposer may accept several addresses of one view keeps the per-row route
 * (ibft_verify_certificates_wire and its own walk).
 *
 * Every per-row output — out_nodes, out_rows, out_class and all three masks, out_sender_mask included — may be NULL, and then
 * nothing per row crosses the bus; what is requested equals ibft_verify_certificates_wire's output bit for bit.  Errors: those
 * of that call, in its order; IBFT_E_INVAL for a NULL out_n_certs or a NULL out_cert with n > 0.  A refused call writes
 * nothing to any out buffer.                                                                                         */
#define IBFT_CERT_NO_RECORD 0xFFFFFFFFu
#define IBFT_CERT_BIT_SENDER 0x01u          /* bits: the row's own IsValidValidator bit                  */
#define IBFT_CERT_BIT_HASH 0x02u            /*       its hash bit                                        */
#define IBFT_CERT_BIT_SELF 0x04u            /*       its self bit                                        */
#define IBFT_CERT_BIT_HAS_PROPOSAL 0x08u    /*       IBFT_CERT_HAS_PROPOSAL of its node                  */
#define IBFT_CERT_BIT_HAS_CERTIFICATE 0x10u /*       IBFT_CERT_HAS_CERTIFICATE of its node               */
typedef struct {
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
} ibft_cert_verdict_t; /* 128 bytes */
int ibft_judge_certificates_wire(ibft_ctx *ctx, const uint8_t *wire, const uint32_t *off, size_t n, size_t rows_cap,
                                 size_t certs_cap, size_t *out_n_rows, size_t *out_n_certs, ibft_cert_verdict_t *out_cert,
                                 ibft_cert_node_t *out_nodes, ibft_wire_row_t *out_rows, uint8_t *out_class,
                                 uint64_t *out_sender_mask, uint64_t *out_hash_mask, uint64_t *out_self_mask);

/* ---- certificates decided: a proposer table on the device -----------------------------------------------------------
 * The records above stop at "pc == 1: valid up to the proposer rule", because IsProposer is the Backend's.  For a Backend whose
 * IsProposer is a pure function of (height, round) that accepts ONE address — the contract the records already rest on — the
 * caller can hand the device that function as a table, and the device finishes validPC, the round-change rule and the
 * proposal rule, the closing IsValidProposalHash(Proposal{raw, maxRound}, hash) of validateProposal (core/ibft.go:780-787)
 * included.
 *
 * ibft_set_proposers installs the proposer of rounds [first_round, first_round + n_rounds) of ONE height, 20 bytes per round
 * (proposer20[20·k .. 20·k + 20) = the proposer of round first_round + k).  It REPLACES the previous table; n_rounds == 0
 * clears it.  The table is copied on the context's stream: calls enqueued before it keep the table they saw.
 * ibft_set_validators does not touch the table — a caller whose proposers follow from the validator set installs it again when
 * the set changes.  Errors: IBFT_E_INVAL for a NULL ctx, a NULL proposer20 with n_rounds > 0, or first_round + n_rounds past
 * 2^64; IBFT_E_TOOBIG for n_rounds > IBFT_PROPOSER_ROUNDS_MAX.  A refused call leaves the earlier table in place.
 * ibft_proposers_info reports the installed range (all zero: no table); any out pointer may be NULL.
 *
 *   T(h, r)                          UNKNOWN when there is no table, h is not the table's height, or r lies outside its range;
 *                                    the entry otherwise.
 *   IsProposer(who, who_len, h, r)   undecided when T(h, r) is UNKNOWN; true when who_len == 20 and the bytes are T(h, r)'s;
 *                                    false otherwise.
 *
 * ibft_decide_certificates_wire is ibft_judge_certificates_wire with one more output: out_decision (certs_cap entries; NULL with
 * n > 0: IBFT_E_INVAL), out_decision[i] belonging to out_cert[i].  Every output the judge call has, out_cert included, is bit
 * for bit the judge call's for the same input; errors are the judge call's in its order; a refused call writes nothing.
 * Values: −1 undecided here, 0 false, 1 true.
 *
 *   valid_pc      validPC whole: the record's pc when pc != 1 (so 2 = no certificate stays 2); for pc == 1
 *                 IsProposer(pc_from, 20, H, pc_round), H = the record's own height for a level-0 record and the parent
 *                 PREPREPARE's height for a record of its RoundChangeCertificate.  ("No PREPARE from the proposer" follows from
 *                 unique senders, as argued above.)
 *   round_change  for a level-0 record whose row is a judged ROUND_CHANGE, handleRoundChangeMessage's closure: valid_pc, and
 *                 for valid_pc == 2: 0 when bits & IBFT_CERT_BIT_HAS_PROPOSAL, else 1.  −1 for every other record.
 *   proposal      −1 for records of level 1 and for level-0 records that are no regular PREPREPARE (class 0, judged, with a
 *                 view, type PREPREPARE, payload PREPREPARE).  Otherwise the clauses below in the reference's order; the first
 *                 one that is not true decides — false: 0, undecided: −1:
 *                   (a) the message carries a Proposal;  (b) Proposal.round == the message's round;
 *                   (c) IsProposer(from, from_len, height, round);  (d) the self bit;
 *                   (e) round == 0: 1 here (validateProposal0 never looks at a certificate);
 *                   (f) rcc: 2 and 0 are false, −1 undecided;
 *                   (g) every record of the certificate has valid_pc != −1;
 *                   (h) no record of the certificate has valid_pc == 1: 1 here;
 *                   (i) among those with valid_pc == 1 the highest pc_round wins, the LAST among equals:
 *                       keccak256(rawProposal ‖ BE64(prepared_round)) == prepared_hash.
 *                 Whenever (i) is reached — whether the hashes agree or not — flags has IBFT_CERT_DECISION_HAS_PREPARED,
 *                 prepared_record is the winner's index in out_cert, prepared_round / prepared_hash its pc_round / pc_hash;
 *                 otherwise they are 0, IBFT_CERT_NO_RECORD and zeros.  The hash of (i) costs one or two Keccak permutations
 *                 whatever the proposal's length: the call keeps the sponge state it had behind the full blocks of
 *                 rawProposal when it computed the self bit.  A proposal beyond IBFT_CERT_DIGEST_MAX_BYTES has class
 *                 IBFT_CERT_CLASS_PROPOSAL_BY_HOST, so its proposal is −1.
 *
 * Left to the caller: the message's view against its own current view (both are in the record), IsValidProposal(raw), and
 * "this node is not the proposer".  Without a table every IsProposer is undecided: the call is the judge call plus −1s, never
 * wrong.  IBFT_FLAG_CERT_DEDUP and both settings of IBFT_CERT_OVERLAP change no byte of out_decision.  With kernel timing on,
 * ibft_last_kernel_ms after this call is the time of the record kernels plus the decision kernels (one more launch pair than
 * after the judge call).  No new ibft_version(): a build without the symbols simply lacks them.                          */
#define IBFT_PROPOSER_ROUNDS_MAX 4096u
int ibft_set_proposers(ibft_ctx *ctx, uint64_t height, uint64_t first_round, const uint8_t *proposer20, size_t n_rounds);
int ibft_proposers_info(ibft_ctx *ctx, uint64_t *height, uint64_t *first_round, uint32_t *n_rounds);
#define IBFT_CERT_DECISION_HAS_PREPARED 0x01u
typedef struct {
  int8_t valid_pc, round_change, proposal; /* −1 undecided here, 0 false, 1 true; valid_pc also 2 */
  uint8_t flags;
  uint32_t prepared_record; /* index in out_cert of the winning record, else IBFT_CERT_NO_RECORD */
  uint64_t prepared_round;
  uint8_t prepared_hash[32];
  uint8_t reserved[16]; /* zero */
} ibft_cert_decision_t; /* 64 bytes */
int ibft_decide_certificates_wire(ibft_ctx *ctx, const uint8_t *wire, const uint32_t *off, size_t n, size_t rows_cap,
                                  size_t certs_cap, size_t *out_n_rows, size_t *out_n_certs, ibft_cert_verdict_t *out_cert,
                                  ibft_cert_decision_t *out_decision, ibft_cert_node_t *out_nodes, ibft_wire_row_t *out_rows,
                                  uint8_t *out_class, uint64_t *out_sender_mask, uint64_t *out_hash_mask,
                                  uint64_t *out_self_mask);

/* ---- round changes: one quorum record per (height, round), GetExtendedRCC on the device ---------------------------
 * What handleRoundChangeMessage does with the per-message answers above (core/ibft.go:470-512, messages/messages.go:202-245):
 * per round it takes the ROUND_CHANGE messages the store still holds — one per sender, a later one replacing an earlier one —,
 * keeps those whose closure holds, asks HasQuorum over their senders and returns the highest round ≥ 1 that has one.
 * ibft_decide_round_changes_wire is ibft_decide_certificates_wire with one more input, `query`, and four more outputs: every
 * output the decide call has is byte for byte the decide call's for the same input, errors are the decide call's in its
 * order.  What a refused call writes is what the decide call writes: one refused among the argument checks in front
 * (IBFT_E_INVAL) writes nothing at all; one refused behind them (IBFT_E_TOOBIG, IBFT_E_NOVALSET) has zeroed the three counts
 * *out_n_rows, *out_n_certs and *out_n_rc, as the decide call zeroes its two once its arguments stand, and writes nothing else.
 *
 *   takes part    a level-0 row that is judged (class 0, status OK, with a view), of type ROUND_CHANGE with a ROUND_CHANGE
 *                 payload, with a 20-byte From and its sender bit (IBFT_CERT_BIT_SENDER) set: the message IBFT.AddMessage would
 *                 have stored.  Every other level-0 row — a PREPREPARE root, a row the tree hands to the host, a row whose
 *                 signature does not verify — has out_rc_view = IBFT_RC_VIEW_NONE (−1), takes no part and supersedes nothing.
 *   key           (height, round) of a row that takes part.  Records are the keys ordered by their lowest such row, ascending.
 *   out_rc_view   n entries: the row's record index, or IBFT_RC_VIEW_OVER (−2) for a key beyond rc_cap — such rows still
 *                 supersede.  *out_n_rc = the number of keys, which may exceed rc_cap.
 *   stored        out_rc_stored, ⌈n/64⌉ words, bits past n zero: bit i is set iff row i takes part and no row j > i that takes
 *                 part has the same key and the same From — what a Messages store fed the batch in row order still holds.
 *   record        out_rc[v], v < min(*out_n_rc, rc_cap, n); entries from there up to min(rc_cap, n) are zeroed:
 *                   height, round, first_row (the key's lowest row), rows (that take part), stored_rows;
 *                   yes_rows / open_rows   stored rows whose decision's round_change is 1 / −1;
 *                   tally                  with S_yes the From column of the stored rows with round_change == 1, in row order:
 *                                          field for field what ibft_tally(S_yes, all-ones) returns on this context (u64 and
 *                                          u256 sets, cold and warm);
 *                   open_power_lo / _hi    the power ibft_tally(S_open, all-ones) reports for the stored rows with
 *                                          round_change == −1 (low 128 bits);
 *                   has_quorum             1 when tally.has_quorum; 0 when the powers of S_yes and S_open TOGETHER stay below
 *                                          the quorum (compared exactly, in full width); −1 otherwise.  Undecided never hides
 *                                          a false and never claims a true.
 *   answer        for `query` = {height, round: the node's view; has_accepted_proposal: 0 or 1; min_round; reserved: 0}; query
 *                 or out_answer NULL: no answer is computed.  R = the records of query.height with round ≥ 1 (GetExtendedRCC's
 *                 accumulator highestRound starts at 0, so round 0 never wins), without the record of query.round when
 *                 has_accepted_proposal is set; r1 = the highest round of R with has_quorum == 1, ru = the highest with −1.
 *                   extended            1: r1 exists and no ru lies above it; −1: an ru above r1, or an ru and no r1; else 0.
 *                   record, round       those of r1, or IBFT_CERT_NO_RECORD and 0.  The RoundChangeCertificate's messages are
 *                                       the stored rows of `record` whose round_change is 1.
 *                   most_record, most_round, most_rows   GetMostRoundChangeMessages(min_round, height): the record of
 *                                       query.height with round ≥ max(min_round, 1) that has the most stored_rows, the LOWEST
 *                                       round among equals (the reference's answer among equals depends on Go's map order,
 *                                       and it answers nothing where round 0 holds the most: its callers ask from round 1
 *                                       up); IBFT_CERT_NO_RECORD, 0, 0 when there is none.
 *                   records_of_height   records of query.height.
 *                   unjudged_rows       level-0 rows of class != 0: the tree left them to the host, the caller still owes
 *                                       them the host route.
 *                   flags               IBFT_RC_OVER when *out_n_rc > rc_cap: the answer covers the records that fit.
 *                                       rc_cap = n always fits.
 *
 * ONE SET, ONE TABLE.  Like every certificate call this one knows one validator set and one proposer table: keys of other
 * heights are formed and tallied under that set, and where their round_change is −1 for want of a table they show it in
 * open_rows.  Every output is a pure function of the batch, the set, the table, the query and rc_cap: nothing depends on thread
 * order, table size or salt.  IBFT_FLAG_CERT_DEDUP and both settings of IBFT_CERT_OVERLAP change no byte of the new outputs.
 *
 * out_rc_view, out_rc_stored and out_answer may be NULL.  IBFT_E_INVAL, with the argument checks in front: a NULL out_n_rc; with
 * n > 0 a NULL out_rc or rc_cap == 0; a query with has_accepted_proposal > 1 or reserved != 0.  An rc_cap above n behaves as n.
 * IBFT_ROUND_CHANGE_SLOTS=<n> (tests only, read at ibft_ctx_create) lowers the slot count of the call's tables, never below the
 * first power of two above n.  No new ibft_version(): a build without the symbol simply lacks it.                     */
#define IBFT_RC_VIEW_NONE (-1)
#define IBFT_RC_VIEW_OVER (-2)
#define IBFT_RC_OVER 1u
typedef struct {
  uint64_t height, round; /* the node's view */
  uint64_t min_round;     /* GetMostRoundChangeMessages */
  uint32_t has_accepted_proposal; /* 0 or 1 */
  uint32_t reserved;      /* zero */
} ibft_rc_query_t; /* 32 bytes */
typedef struct {
  uint64_t height, round;
  uint32_t first_row, rows, stored_rows, yes_rows, open_rows;
  int8_t has_quorum; /* −1 undecided here, 0 false, 1 true */
  uint8_t pad[3];
  uint64_t open_power_lo, open_power_hi;
  ibft_tally_t tally;
  uint8_t reserved[16]; /* zero */
} ibft_rc_record_t; /* 128 bytes */
typedef struct {
  int8_t extended; /* −1 undecided here, 0 false, 1 true */
  uint8_t pad[3];
  uint32_t flags; /* IBFT_RC_OVER */
  uint32_t record, most_record;
  uint64_t round, most_round;
  uint32_t most_rows, records_of_height, unjudged_rows;
  uint8_t reserved[20]; /* zero */
} ibft_rc_answer_t; /* 64 bytes */
int ibft_decide_round_changes_wire(ibft_ctx *ctx, const uint8_t *wire, const uint32_t *off, size_t n, size_t rows_cap,
                                   size_t certs_cap, size_t *out_n_rows, size_t *out_n_certs, ibft_cert_verdict_t *out_cert,
                                   ibft_cert_decision_t *out_decision, ibft_cert_node_t *out_nodes, ibft_wire_row_t *out_rows,
                                   uint8_t *out_class, uint64_t *out_sender_mask, uint64_t *out_hash_mask,
                                   uint64_t *out_self_mask, const ibft_rc_query_t *query, int32_t *out_rc_view,
                                   uint64_t *out_rc_stored, ibft_rc_record_t *out_rc, size_t rc_cap, size_t *out_n_rc,
                                   ibft_rc_answer_t *out_answer);

/* ---- certificates: identical nested messages (IBFT_FLAG_CERT_DEDUP) ----------------------------------------------
 * After a prepared round every ROUND_CHANGE carries a PreparedCertificate built from the same few messages, each signed once
 * and byte-identical wherever it is nested: O(N²) rows, O(N) distinct signatures.  With the flag on, the signature work of
 * the two certificate calls is done once per distinct key — digest32 ‖ sig65 ‖ from20, the 117 bytes of a row's verdict
 * columns; From is part of the key although it is hashed into the digest — and every row gets the bit of the LOWEST row
 * with its key.  The sender bit is a pure function of the key, the validator set and the context's flags (cold or warm,
 * with or without IBFT_FLAG_STRICT_LOW_S), so this is exact.
 *
 * THE CONTRACT: with the flag on, every output of both calls is bit for bit the flag-off output — the three masks, nodes,
 * rows, classes, records, *out_n_rows, *out_n_certs, and the error codes in their order —, on cold and on warm contexts,
 * under both settings of IBFT_CERT_OVERLAP.  These may differ, and only these: ibft_last_dispatch, ibft_last_kernel_ms and
 * ibft_cache_stats — they see the smaller launch (the AUTO rule picks its kernel for the distinct rows, keys are learned
 * from the representatives).
 *
 * Only rows without a pre-flag when the verdict launch is enqueued take part; the others keep their verdict 0.  Digests are
 * still computed per occurrence.  With two verdict launches (the deferred rows — the messages that carry certificates,
 * whose digests arrive later from the side stream — get a small launch of their own) the FIRST launch is deduplicated; the
 * deferred rows are judged per occurrence as before: in these workloads they are distinct messages.  A batch crafted to
 * collide in the dedup table costs a bounded number of key compares per row (128) and is then verified row by row, as
 * without the flag: correctness never rests on a match being found.
 *
 * ibft_cert_stats reports on the LAST certificate call of the context that succeeded: rows = the tree's rows; judged_rows =
 * rows that took part in a verdict launch (no pre-flag); verdict_rows = rows actually given to the verdict kernels;
 * unplaced_rows = rows that gave up on the dedup table and were judged on their own.  Flag off: verdict_rows ==
 * judged_rows, unplaced_rows == 0.  Any pointer may be NULL; a NULL ctx: IBFT_E_INVAL; all zero before the first
 * certificate call.  IBFT_CERT_DEDUP_SLOTS=<n> (tests only, read at ibft_ctx_create) caps the table's slots.  No new
 * ibft_version(): a build without the symbol simply lacks it.                                                       */
int ibft_cert_stats(ibft_ctx *ctx, uint32_t *rows, uint32_t *judged_rows, uint32_t *verdict_rows, uint32_t *unplaced_rows);

/* ---- f4: the signing side, for SIMULATORS ----------------------------------
 * Replaces, for a process that plays n validators at once, the n calls of Backend.BuildCommitMessage
 * (/root/reference/core/backend.go:12-34; sendCommitMessage, core/ibft.go:898-909) that each produce one
 * committed seal: row i gets the 65-byte seal r ‖ s ‖ v of hash32[i] under the secp256k1 key sk32[i]
 * (32 bytes big-endian, must lie in [1, n)), always low-s, v = parity of R.y after the low-s flip — i.e. a
 * seal ibft_verify_seals accepts under every flag — and the signer address keccak256(X‖Y)[12..32) of that
 * key.  out_signer20 and out_ok may be NULL; out_ok[i] = 0 (zero signature, zero address) for a refused key.
 * The nonce is deterministic: k = keccak256(sk ‖ hash ‖ LE32(ctr)) mod n with the first usable ctr
 * (go-ibft_amd/csrc/sign_dev.h) — the CPU oracle's rule, so device seals are byte-identical to the
 * oracle's; it is not RFC 6979 (ibft_sign_seals_ex has that rule).  NOT for a production validator's key: keys cross PCIe in the clear and sit
 * in HBM for the duration of the call (the column is zeroed before the call returns), and the kernel is not
 * written to be constant-time.  On return the batch is STAGED (hash32 / sig65 / signer20 columns are resident
 * exactly as after ibft_seals_stage): ibft_seals_run verifies what was just signed without another upload.  */
int ibft_sign_seals(ibft_ctx *ctx, const uint8_t *sk32, const uint8_t *hash32, size_t n, uint8_t *out_sig65,
                    uint8_t *out_signer20, uint8_t *out_ok);
/* The same under a chosen nonce rule; ibft_sign_seals is ibft_sign_seals_ex(…, IBFT_SIGN_NONCE_KECCAK, …).  Everything said
 * above holds for both rules: the seal-digest convention is applied first (the digest a rule sees is the digest the seal
 * signs), the batch is staged on return, the key column is zeroed before the call returns, a refused key gives ok = 0 with a
 * zero signature and a zero address, n = 0 is legal, and the key-handling warning applies word for word.
 *   IBFT_SIGN_NONCE_KECCAK   k = keccak256(sk ‖ digest ‖ LE32(ctr)) mod n — this library's own rule (and its oracle's).
 *   IBFT_SIGN_NONCE_RFC6979  RFC 6979 §3.2 with HMAC-SHA-256 on the device (hlen = qlen = 256): x = sk32 as given,
 *                            h1 = the digest, bits2octets(h1) = h1 mod n; K = 0x00…, V = 0x01…; two rounds of
 *                            K = HMAC_K(V ‖ 0x00 / 0x01 ‖ x ‖ h1 mod n), V = HMAC_K(V); a candidate is V = HMAC_K(V) read as a
 *                            big-endian integer; after an unusable one K = HMAC_K(V ‖ 0x00), V = HMAC_K(V).  No additional
 *                            data (no k' variant).  A candidate is usable when 0 < k < n, r = R.x with 0 < r < n, and s ≠ 0.
 *                            This is what btcec, bitcoinjs and the published secp256k1 RFC 6979 vectors use: such a signer
 *                            reproduces these seals byte for byte (r ‖ s low-s ‖ v).
 * What it is not, as far as the maintainers know: libsecp256k1's nonce_function_rfc6979 feeds the 32 message bytes
 * UNREDUCED into the DRBG, and libsecp256k1 returns recovery ids 2 and 3 for R.x ≥ n where this signer takes the next
 * candidate.  The two therefore agree except for a digest ≥ n or an R.x ≥ n, each of probability ≈ 2^-128 for a hash.  This
 * has NOT been checked against a libsecp256k1 build: none was available where this was written.
 * Checks, in this order: IBFT_E_INVAL for a NULL ctx or a NULL sk32 / hash32 / out_sig65 with n > 0; IBFT_E_INVAL for an
 * unknown `nonce` (ibft_last_error names it); IBFT_E_TOOBIG for n > max_rows.  A refused call writes nothing to the out
 * buffers and leaves the staged batch as it was.  No new ibft_version(): a build without the symbol simply lacks it. */
#define IBFT_SIGN_NONCE_KECCAK  0u  /* ibft_sign_seals' rule */
#define IBFT_SIGN_NONCE_RFC6979 1u
int ibft_sign_seals_ex(ibft_ctx *ctx, const uint8_t *sk32, const uint8_t *hash32, size_t n, uint32_t nonce,
                       uint8_t *out_sig65, uint8_t *out_signer20, uint8_t *out_ok);
/* The signing side one layer up, for SIMULATORS as well: whole PREPARE / COMMIT messages, built, hashed, signed and stored on
 * the device as the wire bytes ibft_verify_senders_wire / ibft_verify_messages_wire read — Backend.BuildPrepareMessage /
 * BuildCommitMessage (/root/reference/core/backend.go:12-34) for n validators at once.  Row i is (sk32[i], type[i] = 1 PREPARE /
 * 2 COMMIT, height[i], round[i], hash32[i]) and becomes, in canonical proto3 (go-ibft_amd/csrc/sign_message_dev.h):
 *     View{height, round} (always present) ‖ From = keccak256(X‖Y)[12..32) of the key ‖ Signature ‖ Type ‖
 *     PrepareMessage{ProposalHash}  or  CommitMessage{ProposalHash, CommittedSeal}
 * with CommittedSeal = sign(sk, D), D = hash32[i] under the context's seal-digest convention (ibft_set_seal_digest) — byte for
 * byte the seal ibft_sign_seals_ex gives for that key, hash and nonce rule — and Signature = sign(sk, keccak256(PayloadNoSig)),
 * PayloadNoSig being the message without its Signature field (the envelope never applies the seal-digest convention).  `nonce`
 * is IBFT_SIGN_NONCE_KECCAK or IBFT_SIGN_NONCE_RFC6979, for both signatures of a row.
 * Outputs: out_off has n + 1 entries, row i is out_wire[out_off[i] .. out_off[i+1]) — the (wire, off, n) triple
 * ibft_verify_senders_wire takes; a row is 129 … 151 bytes (PREPARE) or 196 … 218 bytes (COMMIT), its length depends on type,
 * height and round only, and wire_cap = n · IBFT_SIGN_MESSAGE_MAX always suffices.  out_from20 (n × 20) and out_ok (n) may be
 * NULL.  A key outside [1, n) gives ok = 0 and a row of its NORMAL length with a zero From, a zero Signature and a zero
 * CommittedSeal (the convention of ibft_sign_seals: lengths stay independent of the keys and the bytes stay canonical
 * protobuf; every verifier rejects the row).
 * Checks, in this order: IBFT_E_INVAL for a NULL ctx, or a NULL sk32 / type / height / round / hash32 / out_wire / out_off with
 * n > 0; IBFT_E_INVAL for an unknown `nonce` (ibft_last_error names it); IBFT_E_TOOBIG for n > max_rows; IBFT_E_INVAL for a
 * type other than 1 or 2 (ibft_last_error names the first such row); IBFT_E_TOOBIG for wire_cap smaller than the total
 * length.  A refused call writes nothing to any out buffer; n = 0 is legal and sets out_off[0] = 0.
 * NOT for a production validator's key — the warning of ibft_sign_seals applies word for word: keys cross PCIe in the clear
 * and sit in HBM for the duration of the call (the column is zeroed before the call returns), and the kernel is not written
 * to be constant-time.  Unlike ibft_sign_seals the call leaves NO staged seal batch and NO resident wire batch behind
 * (ibft_seals_run and ibft_wire_stage_seals have nothing to work on until a batch is staged again): the bytes come back to
 * the host, a following verify call uploads them.  No new ibft_version(): a build without the symbol simply lacks it.  */
#define IBFT_SIGN_MESSAGE_MAX 218u   /* longest message this call emits (COMMIT, height = round = 2^64 − 1) */
int ibft_sign_messages_wire(ibft_ctx *ctx, const uint8_t *sk32, const uint8_t *type, const uint64_t *height,
                            const uint64_t *round, const uint8_t *hash32, size_t n, uint32_t nonce,
                            uint8_t *out_wire, size_t wire_cap, uint32_t *out_off,
                            uint8_t *out_from20, uint8_t *out_ok);
/* The signing side two layers up, for SIMULATORS as well: the PREPREPARE / ROUND_CHANGE envelope around a body the caller encoded —
 * Backend.BuildPrePrepareMessage / BuildRoundChangeMessage (/root/reference/core/backend.go:12-34) for n validators at once, as the
 * wire bytes ibft_verify_certificates_wire / ibft_verify_senders_wire read.  Row i is (sk32[i], type[i] = 0 PREPREPARE /
 * 3 ROUND_CHANGE, height[i], round[i], body[body_at[i] .. body_at[i] + body_len[i])); the body is the already-encoded oneof message
 * (PrePrepareMessage / RoundChangeMessage bytes: Proposal, hash, certificates — the nested messages signed before, e.g. by
 * ibft_sign_messages_wire and by this call).  The row becomes, in canonical proto3 (go-ibft_amd/csrc/sign_envelope_dev.h):
 *     View{height, round} (always present) ‖ From = keccak256(X‖Y)[12..32) of the key ‖ Signature ‖ Type (absent for PREPREPARE,
 *     a zero scalar; 20 03 for ROUND_CHANGE) ‖ field 5 / field 8: varint(body_len) ‖ body (emitted even when body_len = 0)
 * with Signature = sign(sk, keccak256(PayloadNoSig)), PayloadNoSig being the message without its Signature field (the envelope
 * never applies the seal-digest convention).  `nonce` is IBFT_SIGN_NONCE_KECCAK or IBFT_SIGN_NONCE_RFC6979.
 * Bodies are named by (body_at, body_len) columns and NOT by the n + 1 offsets of the other calls because rows MAY name the same
 * or overlapping ranges of `body`: the Q round-change senders that carry one PreparedCertificate upload it once.
 * Outputs: out_off has n + 1 entries, row i is out_wire[out_off[i] .. out_off[i+1]); a row's length depends on type, height, round
 * and body_len only (head ≤ 121 bytes + body_len).  out_from20 (n × 20) and out_ok (n) may be NULL.  A key outside [1, n) gives
 * ok = 0 and a row of its NORMAL length with a zero From and a zero Signature; the body is still copied (lengths stay independent of
 * the keys and the bytes stay canonical protobuf; every verifier rejects the row).  A message longer than
 * IBFT_CERT_DIGEST_MAX_BYTES is still signed; ibft_verify_certificates_wire classes it IBFT_CERT_CLASS_DIGEST_BY_HOST.
 * The envelope digest is hashed on the device from the stored bytes, a lane per message or a wavefront per message, chosen by the
 * rule of ibft_proposal_hashes (batch size in messages of the longest one's length); environment IBFT_ENVELOPE_LANES=1|64, read at
 * ibft_ctx_create, pins a form (tests, A/B) as IBFT_PROPOSAL_LANES does.
 * Checks, in this order: IBFT_E_INVAL for a NULL ctx; IBFT_E_INVAL for a NULL sk32 / type / height / round / body_at / body_len /
 * out_wire / out_off with n > 0; IBFT_E_INVAL for a NULL body with body_bytes > 0; IBFT_E_INVAL for an unknown `nonce`
 * (ibft_last_error names it); IBFT_E_TOOBIG for n > max_rows; IBFT_E_INVAL for a type other than 0 or 3 (ibft_last_error names the
 * first such row); IBFT_E_INVAL for a body range that leaves [0, body_bytes) (computed in 64 bits); IBFT_E_TOOBIG when body_bytes
 * or the total output exceeds the context's proposal byte budget (IBFT_PROPOSAL_BYTES_MAX — the device buffers for bodies and
 * output grow on demand up to it and are kept), or the total output exceeds wire_cap.  A refused call writes nothing to any out
 * buffer; n = 0 is legal and sets out_off[0] = 0.
 * NOT for a production validator's key — the warning of ibft_sign_seals applies word for word: keys cross PCIe in the clear
 * and sit in HBM for the duration of the call (the column is zeroed before the call returns), and the kernels are not written
 * to be constant-time.  Like ibft_sign_messages_wire the call leaves NO staged seal batch and NO resident wire batch behind.
 * No new ibft_version(): a build without the symbol simply lacks it.  */
int ibft_sign_envelopes_wire(ibft_ctx *ctx, const uint8_t *sk32, const uint8_t *type, const uint64_t *height,
                             const uint64_t *round, const uint8_t *body, size_t body_bytes,
                             const uint32_t *body_at, const uint32_t *body_len, size_t n, uint32_t nonce,
                             uint8_t *out_wire, size_t wire_cap, uint32_t *out_off,
                             uint8_t *out_from20, uint8_t *out_ok);
/* Block the host until the context's stream is idle.                               */
int ibft_sync(ibft_ctx *ctx);
/* Device canary (diagnostic; no reference counterpart — a Backend may log it at start-up and a bench line carries it):
 * the verdict kernels are bound by VALU issue, so a sick or shared device shows in one number.  Runs a 0.24 ms kernel
 * of independent 8-byte VALU instructions at one wavefront per SIMD (three untimed launches, median of five timed)
 * on the context's stream and reports the wall time per instruction per SIMD: 1.89 ns on a healthy MI355X
 * (profiles/r06b_kernel_ab.txt; the bare instruction stream: 1.78 ns, profiles/r06b_ubench_wave.txt); > 5 % off means every throughput figure of that device is off by as much.   */
int ibft_issue_probe(ibft_ctx *ctx, float *ns_per_inst, float *kernel_ms);

/* ---- multi-GPU (BASELINE configs #4 / #5) -------------------------------------------
 * Rows are independent, so a batch of n_total rows is split into `world` contiguous row ranges whose
 * length is a multiple of 64 (every 64-bit verdict word is owned by one rank; the last rank takes the
 * remainder): rank k verifies rows [lo, hi) of ibft_shard_range on its own device, with the validator
 * table replicated (ibft_set_validators on every context).  The one exchange step the north star names —
 * "RCCL all-reduce over xGMI of the per-message valid-bitmask" — happens INSIDE this library: ONE
 * ncclAllReduce(sum, u64) over
 *   [ K × verdict words of every shard | one distinct-sender bitmap segment per rank | valid rows ]
 * (K = 1 for a seal / sender batch, 2 for a message set: sender words and valid words).  The verdict words are
 * disjoint (sum ≡ OR).  The tally is NOT additive — ValidatorManager.HasQuorum counts a validator once however
 * many of its messages are valid (a set of addresses: /root/reference/core/validator_manager.go:86-92, 147-155),
 * and nothing stops rows of one sender from landing in two shards — so every rank ships the bitmap of the
 * validators its tally counted (⌈n_validators/64⌉ words in its own segment of the buffer; the segments of the
 * ranks are not disjoint as sets, hence one segment per rank instead of one summed bitmap), and after the
 * all-reduce every rank ORs the segments and recomputes power, distinct_senders and has_quorum from the MERGED
 * bitmap — bit for bit what ibft_verify_seals computes for the same rows on one device (tests/test_gpu_comm.py
 * feeds the same sender to both sides of a shard seam).  ibft_tally_t.shard_overlap reports how often that happened.
 * Buffer size: 8 B × (K·⌈n_total/64⌉ + world·⌈n_validators/64⌉ + 1), e.g. 72 KiB for 65 536 rows / validators on
 * 8 devices — latency-bound on any link.  librccl is dlopen()ed on first use (IBFT_RCCL_LIB overrides the name),
 * so single-GPU users never need it.
 *
 * Two ways to drive it:
 *  (1) one process, all GPUs — what a Go Backend would call: ibft_group_create + ibft_group_verify_seals /
 *      _senders / _messages (one host thread per device inside the library);
 *  (2) one process (or thread) per GPU: every rank creates its context, rank 0 calls ibft_comm_unique_id and
 *      hands the 128 bytes to the others (any side channel), everybody calls ibft_comm_init (collective);
 *      per batch: ibft_seals_stage + ibft_seals_launch on the rank's shard, ibft_seals_exchange (asynchronous:
 *      runs on its own stream behind the tally, so it overlaps with the next ibft_seals_launch; at most two
 *      exchanges in flight), ibft_seals_fetch_merged (oldest exchange first) → global mask + merged tally.  */
#define IBFT_COMM_ID_BYTES 128
int ibft_shard_range(uint64_t n_total, uint32_t rank, uint32_t world, uint64_t *lo, uint64_t *hi); /* pure */
/* layout of the exchange buffer (pure): verdict words per rank, bitmap words per rank, u64 slots in all;
 * n_masks = K above.  Any out pointer may be NULL.                                                        */
int ibft_exchange_layout(uint64_t n_total, uint32_t world, uint32_t n_validators, uint32_t n_masks,
                         uint32_t *words_per_rank, uint32_t *seen_words, uint32_t *slots);
/* Load librccl now (IBFT_RCCL_LIB, librccl.so.1, librccl.so, /opt/rocm/lib/librccl.so.1 — first that opens) instead of at the
 * first ibft_comm_* call: a process that will ALSO load another copy of RCCL under the same SONAME (importing torch does)
 * calls this first, so that the library and the HIP runtime it was built for stay a pair.  IBFT_E_RCCL if none opens.     */
int ibft_comm_preload(void);
int ibft_comm_unique_id(uint8_t id[IBFT_COMM_ID_BYTES]);
int ibft_comm_init(ibft_ctx *ctx, const uint8_t id[IBFT_COMM_ID_BYTES], uint32_t rank, uint32_t world);
int ibft_comm_destroy(ibft_ctx *ctx);
int ibft_seals_exchange(ibft_ctx *ctx, uint64_t n_total);
/* out_mask: ⌈n_total/64⌉ words (bit g = verdict of global row g); either pointer may be NULL */
int ibft_seals_fetch_merged(ibft_ctx *ctx, uint64_t *out_mask, ibft_tally_t *tally);
/* What the communicator itself says about this rank (ncclCommCount / ncclCommUserRank / ncclCommCuDevice): lets a
 * benchmark line state that the collective really spans `nranks` devices.  IBFT_E_INVAL without a communicator.  */
int ibft_comm_info(ibft_ctx *ctx, uint32_t *rccl_nranks, uint32_t *rccl_rank, int32_t *rccl_device);

typedef struct ibft_group ibft_group;
/* One context per listed device + the collective over them; max_rows_total = largest n (0 = 65536 per device).
 * Distinct devices: an RCCL communicator.  A list that names a device more than once (several contexts sharing
 * one MI355X — how the sharded path is exercised with world > 1 on a one-GPU box) cannot be an RCCL communicator
 * (one rank per device); the all-reduce is then the library's own sum kernel over the ranks' buffers on rank 0's
 * exchange stream, everything around it — pack, unpack, streams, double buffering — being the same code.
 * IBFT_GROUP_COLLECTIVE=local selects that kernel for distinct devices too (needs peer access from device[0]).  */
int ibft_group_create(const int32_t *devices, uint32_t n_devices, uint32_t flags, uint32_t max_rows_total,
                      ibft_group **out);
void ibft_group_destroy(ibft_group *g);
uint32_t ibft_group_size(const ibft_group *g);
int ibft_group_is_local(const ibft_group *g); /* 1: the library's sum kernel is the collective, 0: RCCL */
ibft_ctx *ibft_group_ctx(ibft_group *g, uint32_t i); /* the i-th device's context (diagnostics, ibft_last_tally_wide) */
int ibft_group_set_validators(ibft_group *g, uint64_t height, const uint8_t *addrs20, const uint64_t *power, size_t n);
int ibft_group_set_validators_u256(ibft_group *g, uint64_t height, const uint8_t *addrs20, const uint8_t *power_be32,
                                   size_t n);
int ibft_group_set_seal_digest(ibft_group *g, uint32_t mode, const uint8_t *suffix, size_t suffix_len);
/* IsValidCommittedSeal + HasQuorum for n rows sharded over the group's devices: same arguments and results as
 * ibft_verify_seals, out_mask / tally are the merged (global) ones — identical to ibft_verify_seals on the whole
 * batch whatever the rows contain (duplicated senders across shards included).                              */
int ibft_group_verify_seals(ibft_group *g, const uint8_t *hash32, const uint8_t *sig65, const uint8_t *signer20,
                            const uint8_t *pre_flags, size_t n, uint64_t *out_mask, ibft_tally_t *tally);
/* IsValidValidator + HasQuorum, sharded: ibft_verify_senders' arguments and results.                        */
int ibft_group_verify_senders(ibft_group *g, const uint8_t *payload, const uint32_t *off, const uint8_t *sig65,
                              const uint8_t *from20, const uint8_t *pre_flags, size_t n, uint64_t *out_mask,
                              ibft_tally_t *tally);
/* A whole PREPARE / COMMIT set sharded by MESSAGE: ibft_verify_messages' arguments and results (BASELINE config #3's
 * sequence at validator counts beyond one device's batch); the exchange carries both verdict arrays (K = 2).  */
int ibft_group_verify_messages(ibft_group *g, const uint8_t *payload, const uint32_t *off, const uint8_t *msg_sig65,
                               const uint8_t *from20, const uint8_t *hash32, const uint8_t *hash_len,
                               const uint8_t *seal65, const uint8_t *sender_pre, const uint8_t *valid_pre, size_t n,
                               const uint8_t *raw, size_t raw_len, uint64_t round, const uint8_t *digest32,
                               const uint8_t *proposer20, uint64_t *out_sender_mask, uint64_t *out_valid_mask,
                               ibft_tally_t *tally);
/* Certificate trees sharded by CARRIER: device k expands and judges the trees of its own contiguous range of the call's n
 * messages, all devices at once; ibft_verify_certificates_wire's arguments and results, the rows numbered as ONE call over
 * all n messages numbers them (breadth first).  Verdicts are per row and no tally is taken, so the devices exchange
 * nothing.  rows_cap bounds the merged tree and each device's share of it.                                          */
int ibft_group_verify_certificates_wire(ibft_group *g, const uint8_t *wire, const uint32_t *off, size_t n, size_t rows_cap,
                                        size_t *out_n_rows, ibft_cert_node_t *out_nodes, ibft_wire_row_t *out_rows,
                                        uint8_t *out_class, uint64_t *out_sender_mask, uint64_t *out_hash_mask,
                                        uint64_t *out_self_mask);

#ifdef __cplusplus
}
#endif
#endif
