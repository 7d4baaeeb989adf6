//go:build ibftgpu

// Package ibftgpu is the thin cgo binding of libibftgpu.so (include/ibftgpu.h).
//
// NOT COMPILED IN THIS REPOSITORY'S CI: the build image has no Go toolchain.  It is the
// reference-side stub a go-ibft maintainer adds; the C side it binds is exercised through the
// same C ABI by tests/ (ctypes) and by go-ibft_amd/host (C++).  tools/check_go_shim.py checks that
// every identifier these files use exists — in this tree, in include/ibftgpu.h or in the reference.
//
// Placement: shim/go/ is an OVERLAY on the go-ibft module root — shim/go/ibftgpu → <module>/ibftgpu
// (import path github.com/0xPolygon/go-ibft/ibftgpu), shim/go/core/*.go → core/, shim/go/messages/*.go →
// messages/ — with include/ibftgpu.h copied next to this file and libibftgpu.so on the linker /
// loader path (CGO_LDFLAGS=-L…, LD_LIBRARY_PATH).
//
// cgo rules honoured: every slice handed to C is a flat []byte/[]uint32/[]uint64 without Go
// pointers inside; C copies it to HBM before returning and retains nothing.
package ibftgpu

/*
#cgo CFLAGS: -I${SRCDIR}
#cgo LDFLAGS: -libftgpu
#include <stdlib.h>
#include "ibftgpu.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"math/big"
	"runtime"
	"sync"
	"unsafe"
)

// ErrFallback tells the caller to run its own per-message Verifier for this batch.
// The library never synthesises verdicts on failure (all-false stalls liveness,
// all-true breaks safety).
var ErrFallback = errors.New("ibftgpu: device path unavailable, use the CPU verifier")

const (
	RowNil     = C.IBFT_ROW_NIL
	RowBadLen  = C.IBFT_ROW_BADLEN
	RowHashBad = C.IBFT_ROW_HASH_BAD
)

// Tally mirrors ibft_tally_t (ValidatorManager.HasQuorum over the valid rows).
type Tally struct {
	QuorumLo, QuorumHi uint64
	PowerLo, PowerHi   uint64
	ValidRows          uint32
	DistinctSenders    uint32
	HasQuorum          bool
	// sharded calls: how often a validator had valid rows in more than one shard (it is counted once)
	ShardOverlap uint32
	// HasPrepareQuorum calls (a proposer was given): valid rows sent BY the proposer — any such row makes HasQuorum false
	// (core/validator_manager.go:114-121)
	ProposerRows uint32
}

// Ctx owns one ibft_ctx (one HIP stream, resident columns on one GPU).  Use one Ctx per
// concurrent caller — AddMessage goroutines, the round goroutine and the two watcher goroutines of
// core/ibft.go:335-347 — from a FIXED set (a buffered channel of contexts, not a sync.Pool: the validator
// table and the key cache live in the context, so SetValidators must reach every one of them and none
// may be dropped by the garbage collector; INTEGRATION.md §2).
type Ctx struct {
	h *C.ibft_ctx
	// the Go slices of a batch handed to SealsStageNext: the library's copy stream reads them AFTER the cgo call has
	// returned, so they are pinned (runtime.Pinner: the collector neither moves nor frees them) until SealsSwap has waited
	// for that copy
	next runtime.Pinner
	// the batches of BlockSealsSubmit not yet collected, oldest first (their columns stay reachable until then)
	blocks []*blockBatch
}

// Options mirrors ibft_cfg.  KeyCache turns on the warm path (IBFT_FLAG_PUBKEY_CACHE): the
// first valid signature of a validator teaches the device its public key, later ones are verified
// against a per-validator table in HBM (655 KB per validator) — identical verdicts, 4-10x less work.
type Options struct {
	Device     int
	MaxRows    uint32
	StrictLowS bool
	KeyCache   bool
	CertDedup  bool // FlagCertDedup: certificate calls judge each distinct (digest, signature, From) once
	WireRecode bool // FlagWireRecode: the flat wire calls also judge non-canonical PREPARE / COMMIT encodings
}

// FlagCertDedup is IBFT_FLAG_CERT_DEDUP (Options.CertDedup sets it; the environment variable IBFT_CERT_DEDUP=0|1 overrides it).
const FlagCertDedup = uint32(C.IBFT_FLAG_CERT_DEDUP)

// FlagWireRecode is IBFT_FLAG_WIRE_RECODE (Options.WireRecode sets it; the environment variable IBFT_WIRE_RECODE=0|1 overrides
// it): VerifySendersWire / VerifyMessagesWire judge a PREPARE / COMMIT message whose encoding is not the canonical one — fields
// out of order, padded varints, explicit defaults, repeated fields: the recode class of include/ibftgpu.h — as its canonical
// re-encoding instead of marking it WireNeedsHost.  Off by default.
const FlagWireRecode = uint32(C.IBFT_FLAG_WIRE_RECODE)

// abiVersion is what this binding was written against (include/ibftgpu.h: ibft_version; 2 = ibft_tally_t with
// proposer_rows, 56 bytes: an older library would write a shorter struct; 3 = the staged / pipelined pass calls,
// ibft_seals_rows, ibft_issue_probe: a version-2 library lacks symbols this file links against; 4 = ibft_pipeline_stats).
const abiVersion = 4

func New(o Options) (*Ctx, error) {
	if v := int(C.ibft_version()); v < abiVersion {
		return nil, fmt.Errorf("%w: libibftgpu ABI version %d, binding needs >= %d", ErrFallback, v, abiVersion)
	}
	cfg := C.ibft_cfg{device: C.int32_t(o.Device), max_rows: C.uint32_t(o.MaxRows)}
	if o.StrictLowS {
		cfg.flags |= C.IBFT_FLAG_STRICT_LOW_S
	}
	if o.KeyCache {
		cfg.flags |= C.IBFT_FLAG_PUBKEY_CACHE
	}
	if o.CertDedup {
		cfg.flags |= C.IBFT_FLAG_CERT_DEDUP
	}
	if o.WireRecode {
		cfg.flags |= C.IBFT_FLAG_WIRE_RECODE
	}
	var h *C.ibft_ctx
	if rc := C.ibft_ctx_create(&cfg, &h); rc != C.IBFT_OK {
		return nil, fmt.Errorf("%w: %s", ErrFallback, C.GoString(C.ibft_strerror(rc)))
	}
	c := &Ctx{h: h}
	runtime.SetFinalizer(c, (*Ctx).Close)
	return c, nil
}

func (c *Ctx) Close() {
	if c.h != nil {
		C.ibft_ctx_destroy(c.h) // (drains the context's streams: nothing reads the pinned slices any more)
		c.h = nil
	}
	c.next.Unpin()
	for _, b := range c.blocks {
		b.pin.Unpin()
	}
	c.blocks = nil
}

// SetSealDigest tells the context WHAT a committed seal signs in this Backend (core/backend.go:53-55 leaves it open):
// suffix == nil: the 32-byte proposalHash itself (the default); otherwise keccak256(proposalHash ‖ suffix) — e.g. a Backend
// that appends byte(proto.MessageType_COMMIT) before hashing passes []byte{2}.  Every a2 route of the context follows
// (seal batches, the seal half of message sets — a1 keeps comparing the carried hash — and the batch signer).
func (c *Ctx) SetSealDigest(suffix []byte) error {
	mode := C.uint32_t(C.IBFT_SEAL_DIGEST_IDENTITY)
	if suffix != nil {
		mode = C.IBFT_SEAL_DIGEST_KECCAK_SUFFIX
	}
	return c.check(C.ibft_set_seal_digest(c.h, mode, ptr8(suffix), C.size_t(len(suffix))))
}

// Handle is the ibft_ctx pointer for another cgo package of this module (hoststore attaches it to the host mirror:
// ibft_host_attach_gpu); the context stays owned by c.
func (c *Ctx) Handle() unsafe.Pointer { return unsafe.Pointer(c.h) }

// HasQuorum = ValidatorManager.HasQuorum over the rows of `mask` (ibft_tally, core/validator_manager.go:77-96).
func (c *Ctx) HasQuorum(sender20 []byte, mask []uint64) (Tally, error) {
	var t C.ibft_tally_t
	rc := C.ibft_tally(c.h, ptr8(sender20), (*C.uint64_t)(unsafe.Pointer(&mask[0])), C.size_t(len(sender20)/20), &t)
	return tally(t), c.check(rc)
}

// HasPrepareQuorum = ValidatorManager.HasPrepareQuorum (ibft_tally_prepare, core/validator_manager.go:99-127): proposer20
// is proposalMessage.From; the caller answers false itself when there is no proposal message (:101-110).
func (c *Ctx) HasPrepareQuorum(sender20 []byte, mask []uint64, proposer20 []byte) (Tally, error) {
	var t C.ibft_tally_t
	rc := C.ibft_tally_prepare(c.h, ptr8(sender20), (*C.uint64_t)(unsafe.Pointer(&mask[0])), C.size_t(len(sender20)/20),
		ptr8(proposer20), &t)
	return tally(t), c.check(rc)
}

func ptr8(b []byte) *C.uint8_t {
	if len(b) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&b[0]))
}

func (c *Ctx) check(rc C.int) error {
	if rc == C.IBFT_OK {
		return nil
	}
	return fmt.Errorf("%w: %s %s", ErrFallback, C.GoString(C.ibft_strerror(rc)), C.GoString(C.ibft_last_error(c.h)))
}

// SetValidators uploads the table GetVotingPowers(height) returned (20-byte addresses, u64
// powers; SetValidatorsBig takes the *big.Int values as they are).
func (c *Ctx) SetValidators(height uint64, addrs20 []byte, power []uint64) error {
	n := len(power)
	var pp *C.uint64_t
	if n > 0 {
		pp = (*C.uint64_t)(unsafe.Pointer(&power[0]))
	}
	return c.check(C.ibft_set_validators(c.h, C.uint64_t(height), ptr8(addrs20), pp, C.size_t(n)))
}

// SetValidatorsBig is SetValidators for map[string]*big.Int as ValidatorBackend.GetVotingPowers returns it
// (core/validator_manager.go:17-31): every power must fit 256 bits (a larger one returns ErrFallback and the
// set stays on the Go path).  Sums and the quorum are kept in 320 bits on the device.
func (c *Ctx) SetValidatorsBig(height uint64, addrs20 []byte, power []*big.Int) error {
	be := make([]byte, 32*len(power))
	for i, p := range power {
		if p.Sign() < 0 || p.BitLen() > 256 {
			return fmt.Errorf("%w: voting power %d does not fit 256 bits", ErrFallback, i)
		}
		p.FillBytes(be[32*i : 32*i+32])
	}
	return c.check(C.ibft_set_validators_u256(c.h, C.uint64_t(height), ptr8(addrs20), ptr8(be), C.size_t(len(power))))
}

// TallyWide is the full-width result of the last tally (ibft_last_tally_wide).
func (c *Ctx) TallyWide() (power, quorum *big.Int, hasQuorum bool, err error) {
	var t C.ibft_tally_wide_t
	if err = c.check(C.ibft_last_tally_wide(c.h, &t)); err != nil {
		return nil, nil, false, err
	}
	return words(t.power[:]), words(t.quorum[:]), t.has_quorum != 0, nil
}

func words(w []C.uint64_t) *big.Int {
	v := new(big.Int)
	for i := len(w) - 1; i >= 0; i-- {
		v.Lsh(v, 64).Or(v, new(big.Int).SetUint64(uint64(w[i])))
	}
	return v
}

// VerifyHashes = IsValidProposalHash over a batch (core/ibft.go:858-861, 938).
func (c *Ctx) VerifyHashes(raw []byte, round uint64, hash32, hashLen []byte) ([]uint64, error) {
	n := len(hashLen)
	mask := make([]uint64, (n+63)/64+1)
	rc := C.ibft_verify_hashes(c.h, ptr8(raw), C.size_t(len(raw)), C.uint64_t(round), ptr8(hash32), ptr8(hashLen),
		C.size_t(n), (*C.uint64_t)(unsafe.Pointer(&mask[0])))
	return mask, c.check(rc)
}

// VerifySeals = IsValidCommittedSeal over a batch (core/ibft.go:943).
func (c *Ctx) VerifySeals(hash32, sig65, signer20, preFlags []byte) ([]uint64, Tally, error) {
	n := len(sig65) / 65
	mask := make([]uint64, (n+63)/64+1)
	var t C.ibft_tally_t
	rc := C.ibft_verify_seals(c.h, ptr8(hash32), ptr8(sig65), ptr8(signer20), ptr8(preFlags), C.size_t(n),
		(*C.uint64_t)(unsafe.Pointer(&mask[0])), &t)
	return mask, tally(t), c.check(rc)
}

// VerifyBlockSeals = IsValidCommittedSeal + HasQuorum for the committed seals of many finalized blocks in one call
// (ibft_verify_block_seals): the seals of block b are rows [sealOff[b], sealOff[b+1]) and sign
// blockHash32[32b:32b+32].  mask bit i is row i's verdict, tallies[b] block b's HasQuorum — what one VerifySeals
// per block returns.  One validator set per call, the context's: a batch that crosses validator-set changes goes through
// SetValidatorSets + VerifyBlockSealsSets instead of being split where the set changes.
func (c *Ctx) VerifyBlockSeals(blockHash32 []byte, sealOff []uint32, sig65, signer20, preFlags []byte) ([]uint64, []Tally, error) {
	if len(sealOff) == 0 {
		return nil, nil, fmt.Errorf("%w: sealOff needs n_blocks + 1 entries", ErrFallback)
	}
	nb := len(sealOff) - 1
	n := int(sealOff[nb])
	if len(blockHash32) < 32*nb || len(sig65) < 65*n || len(signer20) < 20*n || (preFlags != nil && len(preFlags) < n) {
		return nil, nil, fmt.Errorf("%w: columns shorter than sealOff says", ErrFallback)
	}
	mask := make([]uint64, (n+63)/64+1)
	ct := make([]C.ibft_tally_t, nb+1)
	rc := C.ibft_verify_block_seals(c.h, ptr8(blockHash32), (*C.uint32_t)(unsafe.Pointer(&sealOff[0])), C.size_t(nb),
		ptr8(sig65), ptr8(signer20), ptr8(preFlags), (*C.uint64_t)(unsafe.Pointer(&mask[0])), (*C.ibft_tally_t)(unsafe.Pointer(&ct[0])))
	if err := c.check(rc); err != nil {
		return nil, nil, err
	}
	tallies := make([]Tally, nb)
	for b := range tallies {
		tallies[b] = tally(ct[b])
	}
	return mask, tallies, nil
}

// RecoverSeals = ecrecover over a batch of BARE committed seals (ibft_recover_seals): headers that carry only
// []Signature.  signer20[20i:20i+20] is the address recovered from row i (twenty zero bytes where there is none or
// preFlags[i] != 0), vidx[i] its index in the validator set (-1: no member), mask bit i = recovered AND a member, and the
// tally HasQuorum over the distinct member signers.  Always at the cold rate: when the signers are known use VerifySeals.
func (c *Ctx) RecoverSeals(hash32, sig65, preFlags []byte) (signer20 []byte, vidx []int32, mask []uint64, t Tally, err error) {
	n := len(sig65) / 65
	if len(hash32) < 32*n || (preFlags != nil && len(preFlags) < n) {
		return nil, nil, nil, Tally{}, fmt.Errorf("%w: columns shorter than sig65 says", ErrFallback)
	}
	signer20 = make([]byte, 20*n+20)
	vidx = make([]int32, n+1)
	mask = make([]uint64, (n+63)/64+1)
	var ct C.ibft_tally_t
	rc := C.ibft_recover_seals(c.h, ptr8(hash32), ptr8(sig65), ptr8(preFlags), C.size_t(n), ptr8(signer20),
		(*C.int32_t)(unsafe.Pointer(&vidx[0])), (*C.uint64_t)(unsafe.Pointer(&mask[0])), &ct)
	if err := c.check(rc); err != nil {
		return nil, nil, nil, Tally{}, err
	}
	return signer20[:20*n], vidx[:n], mask, tally(ct), nil
}

// RecoverBlockSeals = RecoverSeals for the committed seals of many finalized blocks in one call
// (ibft_recover_block_seals): rows and offsets as VerifyBlockSeals, no signer column; tallies[b] is block b's HasQuorum
// over the signers recovered from its rows.
func (c *Ctx) RecoverBlockSeals(blockHash32 []byte, sealOff []uint32, sig65, preFlags []byte) (signer20 []byte, vidx []int32, mask []uint64, tallies []Tally, err error) {
	if len(sealOff) == 0 {
		return nil, nil, nil, nil, fmt.Errorf("%w: sealOff needs n_blocks + 1 entries", ErrFallback)
	}
	nb := len(sealOff) - 1
	n := int(sealOff[nb])
	if len(blockHash32) < 32*nb || len(sig65) < 65*n || (preFlags != nil && len(preFlags) < n) {
		return nil, nil, nil, nil, fmt.Errorf("%w: columns shorter than sealOff says", ErrFallback)
	}
	signer20 = make([]byte, 20*n+20)
	vidx = make([]int32, n+1)
	mask = make([]uint64, (n+63)/64+1)
	ct := make([]C.ibft_tally_t, nb+1)
	rc := C.ibft_recover_block_seals(c.h, ptr8(blockHash32), (*C.uint32_t)(unsafe.Pointer(&sealOff[0])), C.size_t(nb),
		ptr8(sig65), ptr8(preFlags), ptr8(signer20), (*C.int32_t)(unsafe.Pointer(&vidx[0])),
		(*C.uint64_t)(unsafe.Pointer(&mask[0])), (*C.ibft_tally_t)(unsafe.Pointer(&ct[0])))
	if err := c.check(rc); err != nil {
		return nil, nil, nil, nil, err
	}
	tallies = make([]Tally, nb)
	for b := range tallies {
		tallies[b] = tally(ct[b])
	}
	return signer20[:20*n], vidx[:n], mask, tallies, nil
}

// SetValidatorSets installs a FAMILY of validator sets next to the single set of SetValidators (ibft_set_validator_sets):
// set s is entries [setOff[s], setOff[s+1]) of addrs20 / power, height[s] is informational.  A syncer collects the distinct
// sets of the run of blocks it fetched (GetVotingPowers per height), installs them once and names each block's set by its
// index here.  Installing replaces the previous family whole; a refused install leaves it in place.
func (c *Ctx) SetValidatorSets(height []uint64, setOff []uint32, addrs20 []byte, power []uint64) error {
	if len(setOff) < 2 || len(height) != len(setOff)-1 {
		return fmt.Errorf("%w: setOff needs n_sets + 1 entries, height n_sets", ErrFallback)
	}
	ns := len(setOff) - 1
	n := int(setOff[ns])
	if len(addrs20) < 20*n || len(power) < n {
		return fmt.Errorf("%w: columns shorter than setOff says", ErrFallback)
	}
	var pp *C.uint64_t
	if n > 0 {
		pp = (*C.uint64_t)(unsafe.Pointer(&power[0]))
	}
	return c.check(C.ibft_set_validator_sets(c.h, C.size_t(ns), (*C.uint64_t)(unsafe.Pointer(&height[0])),
		(*C.uint32_t)(unsafe.Pointer(&setOff[0])), ptr8(addrs20), pp))
}

// SetValidatorSetsBig is SetValidatorSets for *big.Int powers (every one must fit 256 bits, as for SetValidatorsBig).
func (c *Ctx) SetValidatorSetsBig(height []uint64, setOff []uint32, addrs20 []byte, power []*big.Int) error {
	if len(setOff) < 2 || len(height) != len(setOff)-1 {
		return fmt.Errorf("%w: setOff needs n_sets + 1 entries, height n_sets", ErrFallback)
	}
	ns := len(setOff) - 1
	n := int(setOff[ns])
	if len(addrs20) < 20*n || len(power) < n {
		return fmt.Errorf("%w: columns shorter than setOff says", ErrFallback)
	}
	be := make([]byte, 32*n)
	for i, p := range power[:n] {
		if p.Sign() < 0 || p.BitLen() > 256 {
			return fmt.Errorf("%w: voting power %d does not fit 256 bits", ErrFallback, i)
		}
		p.FillBytes(be[32*i : 32*i+32])
	}
	return c.check(C.ibft_set_validator_sets_u256(c.h, C.size_t(ns), (*C.uint64_t)(unsafe.Pointer(&height[0])),
		(*C.uint32_t)(unsafe.Pointer(&setOff[0])), ptr8(addrs20), ptr8(be)))
}

// ValidatorSetsInfo reports the installed family: its sets, the addresses of their union and the device bytes its tables hold.
func (c *Ctx) ValidatorSetsInfo() (sets, unionSize uint32, deviceBytes uint64, err error) {
	var ns, nu C.uint32_t
	var nb C.uint64_t
	err = c.check(C.ibft_validator_sets_info(c.h, &ns, &nu, &nb))
	return uint32(ns), uint32(nu), uint64(nb), err
}

// VerifyBlockSealsSets = VerifyBlockSeals with a validator set PER BLOCK (ibft_verify_block_seals_sets): block b is judged
// under set blockSet[b] of the family SetValidatorSets installed; tallies[b] carries that set's quorum.  Bit for bit what
// SetValidators(set blockSet[b]) + VerifySeals over block b's rows returns, in one call and one verdict launch.
func (c *Ctx) VerifyBlockSealsSets(blockHash32 []byte, sealOff, blockSet []uint32, sig65, signer20, preFlags []byte) ([]uint64, []Tally, error) {
	if len(sealOff) == 0 {
		return nil, nil, fmt.Errorf("%w: sealOff needs n_blocks + 1 entries", ErrFallback)
	}
	nb := len(sealOff) - 1
	n := int(sealOff[nb])
	if len(blockHash32) < 32*nb || len(blockSet) < nb || len(sig65) < 65*n || len(signer20) < 20*n || (preFlags != nil && len(preFlags) < n) {
		return nil, nil, fmt.Errorf("%w: columns shorter than sealOff says", ErrFallback)
	}
	var bs *C.uint32_t
	if nb > 0 {
		bs = (*C.uint32_t)(unsafe.Pointer(&blockSet[0]))
	}
	mask := make([]uint64, (n+63)/64+1)
	ct := make([]C.ibft_tally_t, nb+1)
	rc := C.ibft_verify_block_seals_sets(c.h, ptr8(blockHash32), (*C.uint32_t)(unsafe.Pointer(&sealOff[0])), bs, C.size_t(nb),
		ptr8(sig65), ptr8(signer20), ptr8(preFlags), (*C.uint64_t)(unsafe.Pointer(&mask[0])), (*C.ibft_tally_t)(unsafe.Pointer(&ct[0])))
	if err := c.check(rc); err != nil {
		return nil, nil, err
	}
	tallies := make([]Tally, nb)
	for b := range tallies {
		tallies[b] = tally(ct[b])
	}
	return mask, tallies, nil
}

// RecoverBlockSealsSets = RecoverBlockSeals with a validator set per block (ibft_recover_block_seals_sets): vidx[i] is the
// index of row i's signer in ITS block's set (-1: no member of that set; the address is delivered all the same).
func (c *Ctx) RecoverBlockSealsSets(blockHash32 []byte, sealOff, blockSet []uint32, sig65, preFlags []byte) (signer20 []byte, vidx []int32, mask []uint64, tallies []Tally, err error) {
	if len(sealOff) == 0 {
		return nil, nil, nil, nil, fmt.Errorf("%w: sealOff needs n_blocks + 1 entries", ErrFallback)
	}
	nb := len(sealOff) - 1
	n := int(sealOff[nb])
	if len(blockHash32) < 32*nb || len(blockSet) < nb || len(sig65) < 65*n || (preFlags != nil && len(preFlags) < n) {
		return nil, nil, nil, nil, fmt.Errorf("%w: columns shorter than sealOff says", ErrFallback)
	}
	var bs *C.uint32_t
	if nb > 0 {
		bs = (*C.uint32_t)(unsafe.Pointer(&blockSet[0]))
	}
	signer20 = make([]byte, 20*n+20)
	vidx = make([]int32, n+1)
	mask = make([]uint64, (n+63)/64+1)
	ct := make([]C.ibft_tally_t, nb+1)
	rc := C.ibft_recover_block_seals_sets(c.h, ptr8(blockHash32), (*C.uint32_t)(unsafe.Pointer(&sealOff[0])), bs, C.size_t(nb),
		ptr8(sig65), ptr8(preFlags), ptr8(signer20), (*C.int32_t)(unsafe.Pointer(&vidx[0])),
		(*C.uint64_t)(unsafe.Pointer(&mask[0])), (*C.ibft_tally_t)(unsafe.Pointer(&ct[0])))
	if err := c.check(rc); err != nil {
		return nil, nil, nil, nil, err
	}
	tallies = make([]Tally, nb)
	for b := range tallies {
		tallies[b] = tally(ct[b])
	}
	return signer20[:20*n], vidx[:n], mask, tallies, nil
}

// checkProposals makes the length checks of the three calls that take a batch of proposals: rawOff has one entry more
// than round, raw holds rawOff's last offset.  (Order and start of the offsets are the library's to check.)
func checkProposals(raw []byte, rawOff []uint32, round []uint64) error {
	if len(rawOff) != len(round)+1 {
		return fmt.Errorf("%w: rawOff needs one entry more than round", ErrFallback)
	}
	if len(raw) < int(rawOff[len(round)]) {
		return fmt.Errorf("%w: raw shorter than rawOff says", ErrFallback)
	}
	return nil
}

// ProposalHashes = keccak256(RawProposal ‖ BE64(Round)) of n proposals in one call (ibft_proposal_hashes): proposal i is
// raw[rawOff[i]:rawOff[i+1]] with round[i]; hash32[32i:32i+32] is its proposal hash — what ProposalHash returns for it,
// computed on the device.  For a syncing node that holds (Proposal, []CommittedSeal) pairs and no hashes.
func (c *Ctx) ProposalHashes(raw []byte, rawOff []uint32, round []uint64) (hash32 []byte, err error) {
	if err = checkProposals(raw, rawOff, round); err != nil {
		return nil, err
	}
	n := len(round)
	hash32 = make([]byte, 32*n+32)
	roundCol := make([]uint64, n+1) // (never empty: a pointer to its first entry exists)
	copy(roundCol, round)
	rc := C.ibft_proposal_hashes(c.h, ptr8(raw), (*C.uint32_t)(unsafe.Pointer(&rawOff[0])),
		(*C.uint64_t)(unsafe.Pointer(&roundCol[0])), C.size_t(n), ptr8(hash32))
	if err = c.check(rc); err != nil {
		return nil, err
	}
	return hash32[:32*n], nil
}

// VerifyBlockSealsRaw = VerifyBlockSeals with the blocks' PROPOSALS (raw, rawOff, round as for ProposalHashes, one per
// block) in place of their hashes (ibft_verify_block_seals_raw): the hashes are computed on the device and returned in
// blockHash32 for the caller's own 32-byte compare.
func (c *Ctx) VerifyBlockSealsRaw(raw []byte, rawOff []uint32, round []uint64, sealOff []uint32, sig65, signer20, preFlags []byte) (blockHash32 []byte, mask []uint64, tallies []Tally, err error) {
	if len(sealOff) == 0 {
		return nil, nil, nil, fmt.Errorf("%w: sealOff needs n_blocks + 1 entries", ErrFallback)
	}
	nb := len(sealOff) - 1
	n := int(sealOff[nb])
	if len(round) != nb {
		return nil, nil, nil, fmt.Errorf("%w: one proposal per block", ErrFallback)
	}
	if err = checkProposals(raw, rawOff, round); err != nil {
		return nil, nil, nil, err
	}
	if len(sig65) < 65*n || len(signer20) < 20*n || (preFlags != nil && len(preFlags) < n) {
		return nil, nil, nil, fmt.Errorf("%w: columns shorter than sealOff says", ErrFallback)
	}
	blockHash32 = make([]byte, 32*nb+32)
	mask = make([]uint64, (n+63)/64+1)
	ct := make([]C.ibft_tally_t, nb+1)
	roundCol := make([]uint64, nb+1)
	copy(roundCol, round)
	rc := C.ibft_verify_block_seals_raw(c.h, ptr8(raw), (*C.uint32_t)(unsafe.Pointer(&rawOff[0])),
		(*C.uint64_t)(unsafe.Pointer(&roundCol[0])), (*C.uint32_t)(unsafe.Pointer(&sealOff[0])), C.size_t(nb),
		ptr8(sig65), ptr8(signer20), ptr8(preFlags), ptr8(blockHash32), (*C.uint64_t)(unsafe.Pointer(&mask[0])),
		(*C.ibft_tally_t)(unsafe.Pointer(&ct[0])))
	if err = c.check(rc); err != nil {
		return nil, nil, nil, err
	}
	tallies = make([]Tally, nb)
	for b := range tallies {
		tallies[b] = tally(ct[b])
	}
	return blockHash32[:32*nb], mask, tallies, nil
}

// RecoverBlockSealsRaw = RecoverBlockSeals with the blocks' PROPOSALS in place of their hashes
// (ibft_recover_block_seals_raw); blockHash32 as from VerifyBlockSealsRaw.
func (c *Ctx) RecoverBlockSealsRaw(raw []byte, rawOff []uint32, round []uint64, sealOff []uint32, sig65, preFlags []byte) (blockHash32, signer20 []byte, vidx []int32, mask []uint64, tallies []Tally, err error) {
	if len(sealOff) == 0 {
		return nil, nil, nil, nil, nil, fmt.Errorf("%w: sealOff needs n_blocks + 1 entries", ErrFallback)
	}
	nb := len(sealOff) - 1
	n := int(sealOff[nb])
	if len(round) != nb {
		return nil, nil, nil, nil, nil, fmt.Errorf("%w: one proposal per block", ErrFallback)
	}
	if err = checkProposals(raw, rawOff, round); err != nil {
		return nil, nil, nil, nil, nil, err
	}
	if len(sig65) < 65*n || (preFlags != nil && len(preFlags) < n) {
		return nil, nil, nil, nil, nil, fmt.Errorf("%w: columns shorter than sealOff says", ErrFallback)
	}
	blockHash32 = make([]byte, 32*nb+32)
	signer20 = make([]byte, 20*n+20)
	vidx = make([]int32, n+1)
	mask = make([]uint64, (n+63)/64+1)
	ct := make([]C.ibft_tally_t, nb+1)
	roundCol := make([]uint64, nb+1)
	copy(roundCol, round)
	rc := C.ibft_recover_block_seals_raw(c.h, ptr8(raw), (*C.uint32_t)(unsafe.Pointer(&rawOff[0])),
		(*C.uint64_t)(unsafe.Pointer(&roundCol[0])), (*C.uint32_t)(unsafe.Pointer(&sealOff[0])), C.size_t(nb),
		ptr8(sig65), ptr8(preFlags), ptr8(blockHash32), ptr8(signer20), (*C.int32_t)(unsafe.Pointer(&vidx[0])),
		(*C.uint64_t)(unsafe.Pointer(&mask[0])), (*C.ibft_tally_t)(unsafe.Pointer(&ct[0])))
	if err = c.check(rc); err != nil {
		return nil, nil, nil, nil, nil, err
	}
	tallies = make([]Tally, nb)
	for b := range tallies {
		tallies[b] = tally(ct[b])
	}
	return blockHash32[:32*nb], signer20[:20*n], vidx[:n], mask, tallies, nil
}

// blockBatch keeps the columns of one BlockSealsSubmit reachable — and, where they are Go memory, pinned — until its
// BlockSealsCollect: the library's copy stream reads them after the cgo call has returned.
type blockBatch struct {
	blockHash32, sig65, signer20, preFlags []byte
	sealOff                                []uint32
	blockSet                               []uint32 // the _sets submits: the set of every block
	raw                                    []byte   // the streamed raw forms: the proposals as given,
	rawOff                                 []uint32 // their offsets
	round                                  []uint64 // and the shim's own copy of the rounds
	pin                                    runtime.Pinner
}

func (b *blockBatch) hold(p unsafe.Pointer) {
	if p != nil && !inPinnedBytes(p) { // (PinnedBytes memory is C memory: nothing to pin, and Pinner must not see it)
		b.pin.Pin(p)
	}
}

// BlockSealsSubmit enqueues the batch of VerifyBlockSeals and returns without waiting for the device
// (ibft_block_seals_submit); BlockSealsCollect delivers the OLDEST batch in flight.  At most two batches in flight; per
// step of a chain sync: BlockSealsSubmit(k+1), BlockSealsCollect(k).  The slices must not be written to before the collect
// of their batch; carve them from PinnedBytes for the copy to run under the kernels of the batch before.  Not to be mixed
// with SealsSubmit passes in flight (the library refuses).
func (c *Ctx) BlockSealsSubmit(blockHash32 []byte, sealOff []uint32, sig65, signer20, preFlags []byte) error {
	if len(sealOff) == 0 {
		return fmt.Errorf("%w: sealOff needs n_blocks + 1 entries", ErrFallback)
	}
	nb := len(sealOff) - 1
	n := int(sealOff[nb])
	if len(blockHash32) < 32*nb || len(sig65) < 65*n || len(signer20) < 20*n || (preFlags != nil && len(preFlags) < n) {
		return fmt.Errorf("%w: columns shorter than sealOff says", ErrFallback)
	}
	b := &blockBatch{blockHash32: blockHash32, sealOff: sealOff, sig65: sig65, signer20: signer20, preFlags: preFlags}
	b.hold(unsafe.Pointer(&sealOff[0]))
	b.hold(unsafe.Pointer(ptr8(blockHash32)))
	b.hold(unsafe.Pointer(ptr8(sig65)))
	b.hold(unsafe.Pointer(ptr8(signer20)))
	b.hold(unsafe.Pointer(ptr8(preFlags)))
	rc := C.ibft_block_seals_submit(c.h, ptr8(blockHash32), (*C.uint32_t)(unsafe.Pointer(&sealOff[0])), C.size_t(nb),
		ptr8(sig65), ptr8(signer20), ptr8(preFlags))
	if err := c.check(rc); err != nil {
		b.pin.Unpin() // a refused submit took no slot and reads nothing
		return err
	}
	c.blocks = append(c.blocks, b)
	return nil
}

// BlockSealsPending = batches in flight, rows and blocks of the oldest, as the LIBRARY counts them
// (ibft_block_seals_pending): what BlockSealsCollect sizes its buffers from.
func (c *Ctx) BlockSealsPending() (inFlight, oldestRows, oldestBlocks int, err error) {
	var a, r, b C.uint32_t
	if err = c.check(C.ibft_block_seals_pending(c.h, &a, &r, &b)); err != nil {
		return 0, 0, 0, err
	}
	return int(a), int(r), int(b), nil
}

// BlockSealsCollect waits for the oldest submitted batch only and returns what VerifyBlockSeals returns for it
// (ibft_block_seals_collect); ErrFallback with nothing in flight.
func (c *Ctx) BlockSealsCollect() ([]uint64, []Tally, error) {
	inFlight, n, nb, err := c.BlockSealsPending()
	if err != nil {
		return nil, nil, err
	}
	if inFlight == 0 {
		return nil, nil, ErrFallback // nothing submitted
	}
	mask := make([]uint64, (n+63)/64+1)
	ct := make([]C.ibft_tally_t, nb+1)
	rc := C.ibft_block_seals_collect(c.h, (*C.uint64_t)(unsafe.Pointer(&mask[0])), (*C.ibft_tally_t)(unsafe.Pointer(&ct[0])))
	if err := c.check(rc); err != nil {
		return nil, nil, err
	}
	if len(c.blocks) > 0 { // the batch is delivered: the device has read its columns
		c.blocks[0].pin.Unpin()
		c.blocks[0] = nil
		c.blocks = c.blocks[1:]
	}
	tallies := make([]Tally, nb)
	for b := range tallies {
		tallies[b] = tally(ct[b])
	}
	return mask, tallies, nil
}

// Kinds of a streamed block batch (ibft_block_seals_pending_ex): bit 0 bare seals, signers are emitted; bit 1 proposals were
// given, the computed hashes can be delivered; bit 2 judged under a set per block (the family installed at the submit).
// 0: a batch of BlockSealsSubmit.
const (
	BatchRecover = uint32(C.IBFT_BATCH_RECOVER)
	BatchRaw     = uint32(C.IBFT_BATCH_RAW)
	BatchSets    = uint32(C.IBFT_BATCH_SETS)
)

// submitStreamed is the common part of the streamed submits below: raw == nil && rawOff == nil means hashes given
// (blockHash32), bare means no signer column, sets means a validator set per block (blockSet, one entry per block; the four
// _sets submits).  The slices are held — Go memory pinned, PinnedBytes memory left alone — until the collect of the batch.
func (c *Ctx) submitStreamed(blockHash32, raw []byte, rawOff []uint32, round []uint64, sealOff, blockSet []uint32, sig65, signer20, preFlags []byte, fromRaw, bare, sets bool) error {
	if len(sealOff) == 0 {
		return fmt.Errorf("%w: sealOff needs n_blocks + 1 entries", ErrFallback)
	}
	nb := len(sealOff) - 1
	n := int(sealOff[nb])
	if (sets && len(blockSet) < nb) || len(sig65) < 65*n || (!bare && len(signer20) < 20*n) || (preFlags != nil && len(preFlags) < n) {
		return fmt.Errorf("%w: columns shorter than sealOff says", ErrFallback)
	}
	b := &blockBatch{blockHash32: blockHash32, sealOff: sealOff, blockSet: blockSet, sig65: sig65, signer20: signer20, preFlags: preFlags}
	if fromRaw {
		if len(round) != nb {
			return fmt.Errorf("%w: one proposal per block", ErrFallback)
		}
		if err := checkProposals(raw, rawOff, round); err != nil {
			return err
		}
		b.raw, b.rawOff = raw, rawOff
		b.round = make([]uint64, nb+1) // (never empty: &b.round[0] below; the library reads it until the collect)
		copy(b.round, round)
		b.hold(unsafe.Pointer(ptr8(raw)))
		b.hold(unsafe.Pointer(&rawOff[0]))
		b.hold(unsafe.Pointer(&b.round[0]))
	} else {
		if len(blockHash32) < 32*nb {
			return fmt.Errorf("%w: columns shorter than sealOff says", ErrFallback)
		}
		b.hold(unsafe.Pointer(ptr8(blockHash32)))
	}
	// (every length check is behind us: from here on the only way out without the batch is the refused submit, which unpins)
	b.hold(unsafe.Pointer(&sealOff[0]))
	var bs *C.uint32_t
	if sets {
		bs = blockSetPtr(blockSet, nb)
		b.hold(unsafe.Pointer(bs))
	}
	b.hold(unsafe.Pointer(ptr8(sig65)))
	b.hold(unsafe.Pointer(ptr8(signer20)))
	b.hold(unsafe.Pointer(ptr8(preFlags)))
	off := (*C.uint32_t)(unsafe.Pointer(&sealOff[0]))
	var rc C.int
	switch {
	case sets && fromRaw && !bare:
		rc = C.ibft_block_seals_submit_sets_raw(c.h, ptr8(raw), (*C.uint32_t)(unsafe.Pointer(&rawOff[0])),
			(*C.uint64_t)(unsafe.Pointer(&b.round[0])), off, bs, C.size_t(nb), ptr8(sig65), ptr8(signer20), ptr8(preFlags))
	case sets && fromRaw && bare:
		rc = C.ibft_recover_block_seals_submit_sets_raw(c.h, ptr8(raw), (*C.uint32_t)(unsafe.Pointer(&rawOff[0])),
			(*C.uint64_t)(unsafe.Pointer(&b.round[0])), off, bs, C.size_t(nb), ptr8(sig65), ptr8(preFlags))
	case sets && bare:
		rc = C.ibft_recover_block_seals_submit_sets(c.h, ptr8(blockHash32), off, bs, C.size_t(nb), ptr8(sig65), ptr8(preFlags))
	case sets:
		rc = C.ibft_block_seals_submit_sets(c.h, ptr8(blockHash32), off, bs, C.size_t(nb), ptr8(sig65), ptr8(signer20), ptr8(preFlags))
	case fromRaw && !bare:
		rc = C.ibft_block_seals_submit_raw(c.h, ptr8(raw), (*C.uint32_t)(unsafe.Pointer(&rawOff[0])),
			(*C.uint64_t)(unsafe.Pointer(&b.round[0])), off, C.size_t(nb), ptr8(sig65), ptr8(signer20), ptr8(preFlags))
	case fromRaw && bare:
		rc = C.ibft_recover_block_seals_submit_raw(c.h, ptr8(raw), (*C.uint32_t)(unsafe.Pointer(&rawOff[0])),
			(*C.uint64_t)(unsafe.Pointer(&b.round[0])), off, C.size_t(nb), ptr8(sig65), ptr8(preFlags))
	default:
		rc = C.ibft_recover_block_seals_submit(c.h, ptr8(blockHash32), off, C.size_t(nb), ptr8(sig65), ptr8(preFlags))
	}
	if err := c.check(rc); err != nil {
		b.pin.Unpin() // a refused submit took no slot and reads nothing
		return err
	}
	c.blocks = append(c.blocks, b)
	return nil
}

// BlockSealsSubmitRaw enqueues the batch of VerifyBlockSealsRaw and returns without waiting for the device
// (ibft_block_seals_submit_raw): the streamed pipeline of BlockSealsSubmit — the same two slots — fed with the PROPOSALS.  The
// slices, raw included, must not be written to before the collect of their batch (BlockSealsCollectEx); carve them from
// PinnedBytes for the copy to run under the kernels of the batch before.
func (c *Ctx) BlockSealsSubmitRaw(raw []byte, rawOff []uint32, round []uint64, sealOff []uint32, sig65, signer20, preFlags []byte) error {
	return c.submitStreamed(nil, raw, rawOff, round, sealOff, nil, sig65, signer20, preFlags, true, false, false)
}

// RecoverBlockSealsSubmit enqueues the batch of RecoverBlockSeals (ibft_recover_block_seals_submit): bare seals, streamed.
// Collect it with BlockSealsCollectEx; BlockSealsCollect refuses a recover batch with rows and leaves it in flight.
func (c *Ctx) RecoverBlockSealsSubmit(blockHash32 []byte, sealOff []uint32, sig65, preFlags []byte) error {
	return c.submitStreamed(blockHash32, nil, nil, nil, sealOff, nil, sig65, nil, preFlags, false, true, false)
}

// RecoverBlockSealsSubmitRaw enqueues the batch of RecoverBlockSealsRaw (ibft_recover_block_seals_submit_raw).
func (c *Ctx) RecoverBlockSealsSubmitRaw(raw []byte, rawOff []uint32, round []uint64, sealOff []uint32, sig65, preFlags []byte) error {
	return c.submitStreamed(nil, raw, rawOff, round, sealOff, nil, sig65, nil, preFlags, true, true, false)
}

// blockSetPtr is the block_set column as the C calls take it (nil for a batch without blocks).
func blockSetPtr(blockSet []uint32, nb int) *C.uint32_t {
	if nb == 0 {
		return nil
	}
	return (*C.uint32_t)(unsafe.Pointer(&blockSet[0]))
}

// VerifyBlockSealsSetsRaw = VerifyBlockSealsSets with the blocks' PROPOSALS in place of their hashes
// (ibft_verify_block_seals_sets_raw): ProposalHashes + VerifyBlockSealsSets in one call; blockHash32 as from VerifyBlockSealsRaw.
func (c *Ctx) VerifyBlockSealsSetsRaw(raw []byte, rawOff []uint32, round []uint64, sealOff, blockSet []uint32, sig65, signer20, preFlags []byte) (blockHash32 []byte, mask []uint64, tallies []Tally, err error) {
	if len(sealOff) == 0 {
		return nil, nil, nil, fmt.Errorf("%w: sealOff needs n_blocks + 1 entries", ErrFallback)
	}
	nb := len(sealOff) - 1
	n := int(sealOff[nb])
	if len(round) != nb {
		return nil, nil, nil, fmt.Errorf("%w: one proposal per block", ErrFallback)
	}
	if err = checkProposals(raw, rawOff, round); err != nil {
		return nil, nil, nil, err
	}
	if len(blockSet) < nb || len(sig65) < 65*n || len(signer20) < 20*n || (preFlags != nil && len(preFlags) < n) {
		return nil, nil, nil, fmt.Errorf("%w: columns shorter than sealOff says", ErrFallback)
	}
	blockHash32 = make([]byte, 32*nb+32)
	mask = make([]uint64, (n+63)/64+1)
	ct := make([]C.ibft_tally_t, nb+1)
	roundCol := make([]uint64, nb+1)
	copy(roundCol, round)
	rc := C.ibft_verify_block_seals_sets_raw(c.h, ptr8(raw), (*C.uint32_t)(unsafe.Pointer(&rawOff[0])),
		(*C.uint64_t)(unsafe.Pointer(&roundCol[0])), (*C.uint32_t)(unsafe.Pointer(&sealOff[0])), blockSetPtr(blockSet, nb), C.size_t(nb),
		ptr8(sig65), ptr8(signer20), ptr8(preFlags), ptr8(blockHash32), (*C.uint64_t)(unsafe.Pointer(&mask[0])),
		(*C.ibft_tally_t)(unsafe.Pointer(&ct[0])))
	if err = c.check(rc); err != nil {
		return nil, nil, nil, err
	}
	tallies = make([]Tally, nb)
	for b := range tallies {
		tallies[b] = tally(ct[b])
	}
	return blockHash32[:32*nb], mask, tallies, nil
}

// RecoverBlockSealsSetsRaw = RecoverBlockSealsSets with the blocks' PROPOSALS in place of their hashes
// (ibft_recover_block_seals_sets_raw).
func (c *Ctx) RecoverBlockSealsSetsRaw(raw []byte, rawOff []uint32, round []uint64, sealOff, blockSet []uint32, sig65, preFlags []byte) (blockHash32, signer20 []byte, vidx []int32, mask []uint64, tallies []Tally, err error) {
	if len(sealOff) == 0 {
		return nil, nil, nil, nil, nil, fmt.Errorf("%w: sealOff needs n_blocks + 1 entries", ErrFallback)
	}
	nb := len(sealOff) - 1
	n := int(sealOff[nb])
	if len(round) != nb {
		return nil, nil, nil, nil, nil, fmt.Errorf("%w: one proposal per block", ErrFallback)
	}
	if err = checkProposals(raw, rawOff, round); err != nil {
		return nil, nil, nil, nil, nil, err
	}
	if len(blockSet) < nb || len(sig65) < 65*n || (preFlags != nil && len(preFlags) < n) {
		return nil, nil, nil, nil, nil, fmt.Errorf("%w: columns shorter than sealOff says", ErrFallback)
	}
	blockHash32 = make([]byte, 32*nb+32)
	signer20 = make([]byte, 20*n+20)
	vidx = make([]int32, n+1)
	mask = make([]uint64, (n+63)/64+1)
	ct := make([]C.ibft_tally_t, nb+1)
	roundCol := make([]uint64, nb+1)
	copy(roundCol, round)
	rc := C.ibft_recover_block_seals_sets_raw(c.h, ptr8(raw), (*C.uint32_t)(unsafe.Pointer(&rawOff[0])),
		(*C.uint64_t)(unsafe.Pointer(&roundCol[0])), (*C.uint32_t)(unsafe.Pointer(&sealOff[0])), blockSetPtr(blockSet, nb), C.size_t(nb),
		ptr8(sig65), ptr8(preFlags), ptr8(blockHash32), ptr8(signer20), (*C.int32_t)(unsafe.Pointer(&vidx[0])),
		(*C.uint64_t)(unsafe.Pointer(&mask[0])), (*C.ibft_tally_t)(unsafe.Pointer(&ct[0])))
	if err = c.check(rc); err != nil {
		return nil, nil, nil, nil, nil, err
	}
	tallies = make([]Tally, nb)
	for b := range tallies {
		tallies[b] = tally(ct[b])
	}
	return blockHash32[:32*nb], signer20[:20*n], vidx[:n], mask, tallies, nil
}

// BlockSealsSubmitSets enqueues the batch of VerifyBlockSealsSets (ibft_block_seals_submit_sets): the streamed pipeline of
// BlockSealsSubmit — the same two slots — with a validator set PER BLOCK.  The batch is judged under the family installed at
// the submit: SetValidatorSets for the next run may be called while it is in flight.  Collect with BlockSealsCollect[Ex].
func (c *Ctx) BlockSealsSubmitSets(blockHash32 []byte, sealOff, blockSet []uint32, sig65, signer20, preFlags []byte) error {
	return c.submitStreamed(blockHash32, nil, nil, nil, sealOff, blockSet, sig65, signer20, preFlags, false, false, true)
}

// BlockSealsSubmitSetsRaw enqueues the batch of VerifyBlockSealsSetsRaw (ibft_block_seals_submit_sets_raw): what a syncer that
// holds (Proposal, seals, blockSet) streams across validator-set changes.
func (c *Ctx) BlockSealsSubmitSetsRaw(raw []byte, rawOff []uint32, round []uint64, sealOff, blockSet []uint32, sig65, signer20, preFlags []byte) error {
	return c.submitStreamed(nil, raw, rawOff, round, sealOff, blockSet, sig65, signer20, preFlags, true, false, true)
}

// RecoverBlockSealsSubmitSets enqueues the batch of RecoverBlockSealsSets (ibft_recover_block_seals_submit_sets); collect it
// with BlockSealsCollectEx.
func (c *Ctx) RecoverBlockSealsSubmitSets(blockHash32 []byte, sealOff, blockSet []uint32, sig65, preFlags []byte) error {
	return c.submitStreamed(blockHash32, nil, nil, nil, sealOff, blockSet, sig65, nil, preFlags, false, true, true)
}

// RecoverBlockSealsSubmitSetsRaw enqueues the batch of RecoverBlockSealsSetsRaw (ibft_recover_block_seals_submit_sets_raw).
func (c *Ctx) RecoverBlockSealsSubmitSetsRaw(raw []byte, rawOff []uint32, round []uint64, sealOff, blockSet []uint32, sig65, preFlags []byte) error {
	return c.submitStreamed(nil, raw, rawOff, round, sealOff, blockSet, sig65, nil, preFlags, true, true, true)
}

// BlockSealsPendingEx = BlockSealsPending plus the kind of the oldest batch (ibft_block_seals_pending_ex): BatchRecover /
// BatchRaw / BatchSets bits, 0 for a batch of BlockSealsSubmit.
func (c *Ctx) BlockSealsPendingEx() (inFlight, oldestRows, oldestBlocks int, oldestKind uint32, err error) {
	var a, r, b, k C.uint32_t
	if err = c.check(C.ibft_block_seals_pending_ex(c.h, &a, &r, &b, &k)); err != nil {
		return 0, 0, 0, 0, err
	}
	return int(a), int(r), int(b), uint32(k), nil
}

// BlockBatchResult is what BlockSealsCollectEx delivers: Mask and Tallies always; BlockHash32 (n_blocks × 32, the hashes before
// the seal-digest convention) for a batch submitted raw, nil otherwise; Signer20 (n × 20) and Vidx (n) for a recover batch,
// nil otherwise.
type BlockBatchResult struct {
	Kind        uint32
	BlockHash32 []byte
	Signer20    []byte
	Vidx        []int32
	Mask        []uint64
	Tallies     []Tally
}

// BlockSealsCollectEx waits for the oldest submitted batch of ANY kind and returns what its synchronous sibling returns for it
// (ibft_block_seals_collect_ex); buffers are sized from BlockSealsPendingEx.  ErrFallback with nothing in flight.
func (c *Ctx) BlockSealsCollectEx() (*BlockBatchResult, error) {
	inFlight, n, nb, kind, err := c.BlockSealsPendingEx()
	if err != nil {
		return nil, err
	}
	if inFlight == 0 {
		return nil, ErrFallback // nothing submitted
	}
	res := &BlockBatchResult{Kind: kind, Mask: make([]uint64, (n+63)/64+1)}
	ct := make([]C.ibft_tally_t, nb+1)
	var hashes, signers []byte
	var vidx []int32
	var pv *C.int32_t
	if kind&BatchRaw != 0 {
		hashes = make([]byte, 32*nb+32)
	}
	if kind&BatchRecover != 0 {
		signers = make([]byte, 20*n+20)
		vidx = make([]int32, n+1)
		pv = (*C.int32_t)(unsafe.Pointer(&vidx[0]))
	}
	rc := C.ibft_block_seals_collect_ex(c.h, ptr8(hashes), ptr8(signers), pv, (*C.uint64_t)(unsafe.Pointer(&res.Mask[0])),
		(*C.ibft_tally_t)(unsafe.Pointer(&ct[0])))
	if err := c.check(rc); err != nil {
		return nil, err
	}
	if len(c.blocks) > 0 { // the batch is delivered: the device has read its columns
		c.blocks[0].pin.Unpin()
		c.blocks[0] = nil
		c.blocks = c.blocks[1:]
	}
	if hashes != nil {
		res.BlockHash32 = hashes[:32*nb]
	}
	if signers != nil {
		res.Signer20 = signers[:20*n]
		res.Vidx = vidx[:n]
	}
	res.Tallies = make([]Tally, nb)
	for b := range res.Tallies {
		res.Tallies[b] = tally(ct[b])
	}
	return res, nil
}

// VerifySenders = IsValidValidator over a batch (core/ibft.go:1128); payload is the
// concatenation of msg.PayloadNoSig(), off its n+1 offsets.
func (c *Ctx) VerifySenders(payload []byte, off []uint32, sig65, from20, preFlags []byte) ([]uint64, Tally, error) {
	n := len(off) - 1
	mask := make([]uint64, (n+63)/64+1)
	var t C.ibft_tally_t
	rc := C.ibft_verify_senders(c.h, ptr8(payload), (*C.uint32_t)(unsafe.Pointer(&off[0])), ptr8(sig65), ptr8(from20),
		ptr8(preFlags), C.size_t(n), (*C.uint64_t)(unsafe.Pointer(&mask[0])), &t)
	return mask, tally(t), c.check(rc)
}

// VerifyMessages = a whole PREPARE / COMMIT set in one call (ibft_verify_messages): senderMask bit i is
// IsValidValidator(message i), validMask bit i the handlePrepare / handleCommit closure for it, the tally is
// HasQuorum over the rows with both bits — ValidatorManager.HasPrepareQuorum (core/validator_manager.go:99-127) when
// proposer20 (the accepted proposal message's From) is not nil.  seal65 == nil for a PREPARE set; senderPre / validPre
// may be nil.
func (c *Ctx) VerifyMessages(payload []byte, off []uint32, msgSig65, from20, hash32, hashLen, seal65, senderPre, validPre,
	raw []byte, round uint64, proposer20 []byte) (senderMask, validMask []uint64, t Tally, err error) {
	n := len(off) - 1
	senderMask, validMask = make([]uint64, (n+63)/64+1), make([]uint64, (n+63)/64+1)
	var ct C.ibft_tally_t
	rc := C.ibft_verify_messages(c.h, ptr8(payload), (*C.uint32_t)(unsafe.Pointer(&off[0])), ptr8(msgSig65), ptr8(from20),
		ptr8(hash32), ptr8(hashLen), ptr8(seal65), ptr8(senderPre), ptr8(validPre), C.size_t(n), ptr8(raw),
		C.size_t(len(raw)), C.uint64_t(round), nil, ptr8(proposer20), (*C.uint64_t)(unsafe.Pointer(&senderMask[0])),
		(*C.uint64_t)(unsafe.Pointer(&validMask[0])), &ct)
	return senderMask, validMask, tally(ct), c.check(rc)
}

// Routing byte per raw message (ibft_verify_messages_wire, out_class).
const (
	WireClassNeedsHost = byte(C.IBFT_WIRE_CLASS_NEEDS_HOST)
	WireClassClosure   = byte(C.IBFT_WIRE_CLASS_CLOSURE)
)

// VerifyMessagesWire = raw messages judged completely (ibft_verify_messages_wire): the device walks the bytes and
// verifies both signatures of every PREPARE / COMMIT of the view (height, round) in one launch.
// proposer20 != nil (a batch of PREPAREs of the view): the tally is HasPrepareQuorum.
func (c *Ctx) VerifyMessagesWire(wire []byte, off []uint32, height, round uint64, raw []byte, proposalRound uint64,
	proposer20 []byte) (senderMask, validMask []uint64, class []byte, t Tally, err error) {
	n := len(off) - 1
	senderMask, validMask = make([]uint64, (n+63)/64+1), make([]uint64, (n+63)/64+1)
	class = make([]byte, n+1)
	var ct C.ibft_tally_t
	rc := C.ibft_verify_messages_wire(c.h, ptr8(wire), (*C.uint32_t)(unsafe.Pointer(&off[0])), C.size_t(n), C.uint64_t(height),
		C.uint64_t(round), ptr8(raw), C.size_t(len(raw)), C.uint64_t(proposalRound), nil,
		(*C.uint64_t)(unsafe.Pointer(&senderMask[0])), (*C.uint64_t)(unsafe.Pointer(&validMask[0])), ptr8(class), nil,
		ptr8(proposer20), &ct)
	return senderMask, validMask, class[:n], tally(ct), c.check(rc)
}

// CertNode mirrors ibft_cert_node_t: one IbftMessage of a certificate tree (VerifyCertificatesWire).
type CertNode struct {
	Off, Len              uint32 // the message's bytes in the call's buffer
	Parent, Ordinal       uint32 // containing row (CertNoParent for the call's own messages), position among its children
	FirstChild, NChildren uint32 // its nested messages are rows [FirstChild, FirstChild+NChildren)
	RawOff, RawLen        uint32 // Proposal.rawProposal it carries
	ProposalRound         uint64
	Cut0, Cut1            uint32 // its signature field, relative to Off: PayloadNoSig = bytes minus [Cut0, Cut1)
	Level, Role, Flags    uint8
	_                     [5]byte
}

const (
	CertNoParent         = uint32(C.IBFT_CERT_NO_PARENT)
	CertClassNeedsHost   = byte(C.IBFT_CERT_CLASS_NEEDS_HOST)       // not canonical here: the stock route decides this message
	CertClassDigestHost  = byte(C.IBFT_CERT_CLASS_DIGEST_BY_HOST)   // canonical, longer than the device hashes
	CertClassProposalHost = byte(C.IBFT_CERT_CLASS_PROPOSAL_BY_HOST) // the Proposal it carries is that long
	CertRolePCProposal   = uint8(C.IBFT_CERT_ROLE_PC_PROPOSAL)
	CertRolePCPrepare    = uint8(C.IBFT_CERT_ROLE_PC_PREPARE)
	CertRoleRCCMessage   = uint8(C.IBFT_CERT_ROLE_RCC_MESSAGE)
)

// VerifyCertificatesWire = every IsValidValidator / IsValidProposalHash that validateProposal, validPC and
// handleRoundChangeMessage (core/ibft.go:470-551, 683-788, 1162-1231) ask about the messages NESTED in the given raw
// PREPREPARE / ROUND_CHANGE messages, and about those messages themselves, in one call (ibft_verify_certificates_wire).
// Rows are breadth first: the call's messages, then their nested messages in wire order, and so on — the order in which
// a decoded message lists them.  sender / hash / self are bit masks over the rows, class one routing byte per row.
func (c *Ctx) VerifyCertificatesWire(wire []byte, off []uint32, rowsCap int) (nodes []CertNode, class []byte, sender, hash, self []uint64, err error) {
	n := len(off) - 1
	nodes = make([]CertNode, rowsCap+1)
	class = make([]byte, rowsCap+1)
	sender, hash, self = make([]uint64, (rowsCap+63)/64+1), make([]uint64, (rowsCap+63)/64+1), make([]uint64, (rowsCap+63)/64+1)
	var rows C.size_t
	rc := C.ibft_verify_certificates_wire(c.h, ptr8(wire), (*C.uint32_t)(unsafe.Pointer(&off[0])), C.size_t(n), C.size_t(rowsCap), &rows,
		(*C.ibft_cert_node_t)(unsafe.Pointer(&nodes[0])), nil, ptr8(class), (*C.uint64_t)(unsafe.Pointer(&sender[0])),
		(*C.uint64_t)(unsafe.Pointer(&hash[0])), (*C.uint64_t)(unsafe.Pointer(&self[0])))
	return nodes[:int(rows)], class[:int(rows)], sender, hash, self, c.check(rc)
}

// CertVerdict mirrors ibft_cert_verdict_t: what the reference asks about ONE certificate carrier, decided on the device
// (JudgeCertificatesWire).  PC / RCC: -1 undecided here (decide by the walk over the decoded message), 0 invalid, 1 valid,
// 2 the message carries no certificate.
type CertVerdict struct {
	Row, FirstChild, NChildren uint32 // the carrier's row and its nested messages' rows
	FirstChildCert             uint32 // a root PREPREPARE: index of the record of its first nested ROUND_CHANGE (CertNoRecord: none)
	RCCRows                    uint32 // rows of the certificate's subtree (RCC >= 0)
	PC, RCC                    int8
	Class, Bits                uint8 // the row's routing byte; CertBit*
	Type, Role, Level, FromLen uint8
	Reserved                   uint32
	Height, Round              uint64
	PCRound                    uint64 // PC == 1: view round, From and carried hash of the certificate's proposal message
	From                       [20]byte
	PCFrom                     [20]byte
	PCHash                     [32]byte
}

// The struct is exactly as large as the C one: unsafe.Sizeof is a constant, and a uintptr constant below zero does not compile.
const (
	_ = unsafe.Sizeof(CertVerdict{}) - 128
	_ = 128 - unsafe.Sizeof(CertVerdict{})
)

const (
	CertNoRecord          = uint32(C.IBFT_CERT_NO_RECORD)
	CertBitSender         = uint8(C.IBFT_CERT_BIT_SENDER)
	CertBitHash           = uint8(C.IBFT_CERT_BIT_HASH)
	CertBitSelf           = uint8(C.IBFT_CERT_BIT_SELF)
	CertBitHasProposal    = uint8(C.IBFT_CERT_BIT_HAS_PROPOSAL)
	CertBitHasCertificate = uint8(C.IBFT_CERT_BIT_HAS_CERTIFICATE)
)

// JudgeCertificatesWire = VerifyCertificatesWire's tree, and on top of it validPC and the RoundChangeCertificate rules of
// validateProposal (core/ibft.go:1162-1231, 697-778) decided PER CARRIER on the device (ibft_judge_certificates_wire): one
// record for each of the call's messages and for each ROUND_CHANGE message inside a root PREPREPARE's certificate, in row
// order.  No per-row output crosses the bus.  The caller finishes with IsProposer(PCFrom, height, PCRound) where PC == 1 —
// which rests on IsProposer accepting at most one address per view (include/ibftgpu.h); a Backend without that property
// keeps VerifyCertificatesWire.
func (c *Ctx) JudgeCertificatesWire(wire []byte, off []uint32, rowsCap, certsCap int) (certs []CertVerdict, rows int, err error) {
	n := len(off) - 1
	certs = make([]CertVerdict, certsCap+1)
	var nRows, nCerts C.size_t
	rc := C.ibft_judge_certificates_wire(c.h, ptr8(wire), (*C.uint32_t)(unsafe.Pointer(&off[0])), C.size_t(n), C.size_t(rowsCap),
		C.size_t(certsCap), &nRows, &nCerts, (*C.ibft_cert_verdict_t)(unsafe.Pointer(&certs[0])), nil, nil, nil, nil, nil, nil)
	return certs[:int(nCerts)], int(nRows), c.check(rc)
}

// CertDecision mirrors ibft_cert_decision_t: what the reference decides about the record next to it once IsProposer is
// answered from the table of SetProposers (DecideCertificatesWire).  ValidPC / RoundChange / Proposal: -1 undecided here
// (no table entry for the view, or an irregular shape), 0 false, 1 true; ValidPC also 2, the message carries no certificate.
type CertDecision struct {
	ValidPC, RoundChange, Proposal int8
	Flags                          uint8  // CertDecisionHasPrepared
	PreparedRecord                 uint32 // index of the record whose certificate is the highest prepared round (CertNoRecord: none)
	PreparedRound                  uint64
	PreparedHash                   [32]byte
	Reserved                       [16]byte
}

const (
	_ = unsafe.Sizeof(CertDecision{}) - 64
	_ = 64 - unsafe.Sizeof(CertDecision{})
)

const (
	CertDecisionHasPrepared = uint8(C.IBFT_CERT_DECISION_HAS_PREPARED)
	ProposerRoundsMax       = int(C.IBFT_PROPOSER_ROUNDS_MAX)
)

// SetProposers installs the proposer of rounds [firstRound, firstRound + len(proposers20)/20) of ONE height
// (ibft_set_proposers), 20 bytes per round; it replaces the previous table, an empty slice clears it.  SetValidators leaves
// the table alone: install it again when the validator set changes.  A Backend has only the IsProposer predicate
// (core/backend.go:47-48), so it fills the slice by asking once per validator and round, or from its own proposer calculator.
func (c *Ctx) SetProposers(height, firstRound uint64, proposers20 []byte) error {
	if len(proposers20)%20 != 0 {
		return fmt.Errorf("%w: %d bytes are no whole number of 20-byte addresses", ErrFallback, len(proposers20))
	}
	return c.check(C.ibft_set_proposers(c.h, C.uint64_t(height), C.uint64_t(firstRound), ptr8(proposers20), C.size_t(len(proposers20)/20)))
}

// DecideCertificatesWire = JudgeCertificatesWire, and for every record a decision under the table of SetProposers
// (ibft_decide_certificates_wire): validPC whole, handleRoundChangeMessage's closure for a root ROUND_CHANGE, and for a root
// PREPREPARE validateProposal with its closing IsValidProposalHash (core/ibft.go:640-787).  decisions[i] belongs to certs[i].
// Left to the caller: the message's view against its own, IsValidProposal(raw), and "this node is not the proposer".
func (c *Ctx) DecideCertificatesWire(wire []byte, off []uint32, rowsCap, certsCap int) (certs []CertVerdict, decisions []CertDecision, rows int, err error) {
	n := len(off) - 1
	certs = make([]CertVerdict, certsCap+1)
	decisions = make([]CertDecision, certsCap+1)
	var nRows, nCerts C.size_t
	rc := C.ibft_decide_certificates_wire(c.h, ptr8(wire), (*C.uint32_t)(unsafe.Pointer(&off[0])), C.size_t(n), C.size_t(rowsCap),
		C.size_t(certsCap), &nRows, &nCerts, (*C.ibft_cert_verdict_t)(unsafe.Pointer(&certs[0])),
		(*C.ibft_cert_decision_t)(unsafe.Pointer(&decisions[0])), nil, nil, nil, nil, nil, nil)
	return certs[:int(nCerts)], decisions[:int(nCerts)], int(nRows), c.check(rc)
}

// RCQuery mirrors ibft_rc_query_t: the node's view, whether it has accepted a proposal (0 or 1), and the minRound of
// GetMostRoundChangeMessages.
type RCQuery struct {
	Height, Round       uint64
	MinRound            uint64
	HasAcceptedProposal uint32
	Reserved            uint32
}

// RCTally is ibft_tally_t as it lies inside an RCRecord; Tally() gives it the shape every other call returns.
type RCTally struct {
	QuorumLo, QuorumHi, PowerLo, PowerHi                                        uint64
	ValidRows, DistinctSenders, HasQuorum, ShardOverlap, ProposerRows, Reserved uint32
}

// Tally converts the record's tally.
func (t RCTally) Tally() Tally {
	return Tally{t.QuorumLo, t.QuorumHi, t.PowerLo, t.PowerHi, t.ValidRows, t.DistinctSenders, t.HasQuorum != 0, t.ShardOverlap, t.ProposerRows}
}

// RCRecord mirrors ibft_rc_record_t: one (height, round) that has a stored ROUND_CHANGE message in the batch.  Tally is HasQuorum
// over the stored rows whose closure holds (round_change 1), OpenPower the power of those whose closure is undecided here (-1);
// HasQuorum is 1, 0 or -1: undecided where the open rows could still change the answer.
type RCRecord struct {
	Height, Round                                 uint64
	FirstRow, Rows, StoredRows, YesRows, OpenRows uint32
	HasQuorum                                     int8
	Pad                                           [3]byte
	OpenPowerLo, OpenPowerHi                      uint64
	Tally                                         RCTally
	Reserved                                      [16]byte
}

// RCAnswer mirrors ibft_rc_answer_t: GetExtendedRCC (Extended 1: Record / Round name the winning round, 0: none, -1: undecided
// here) and GetMostRoundChangeMessages (MostRecord, MostRound, MostRows) for the query, the records of its height, the level-0
// rows the tree left to the host, and RCOver in Flags when the batch had more keys than rcCap.
type RCAnswer struct {
	Extended                                int8
	Pad                                     [3]byte
	Flags                                   uint32
	Record, MostRecord                      uint32
	Round, MostRound                        uint64
	MostRows, RecordsOfHeight, UnjudgedRows uint32
	Reserved                                [20]byte
}

const (
	_ = unsafe.Sizeof(RCQuery{}) - 32
	_ = 32 - unsafe.Sizeof(RCQuery{})
	_ = unsafe.Sizeof(RCRecord{}) - 128
	_ = 128 - unsafe.Sizeof(RCRecord{})
	_ = unsafe.Sizeof(RCAnswer{}) - 64
	_ = 64 - unsafe.Sizeof(RCAnswer{})
)

const (
	RCViewNone = int32(C.IBFT_RC_VIEW_NONE)
	RCViewOver = int32(C.IBFT_RC_VIEW_OVER)
	RCOver     = uint32(C.IBFT_RC_OVER)
)

// RoundChangesResult is what DecideRoundChangesWire adds to DecideCertificatesWire: the record of every level-0 row (RCViewNone:
// it takes no part, RCViewOver: its key did not fit rcCap), the stored bits, the records that fit, the number of keys, and the
// answer (nil without a query).
type RoundChangesResult struct {
	View    []int32
	Stored  []uint64
	Records []RCRecord
	Keys    int
	Answer  *RCAnswer
}

// DecideRoundChangesWire = DecideCertificatesWire, and what handleRoundChangeMessage does with its per-message answers
// (ibft_decide_round_changes_wire; core/ibft.go:470-512): per (height, round) the ROUND_CHANGE messages a store fed the batch in
// row order still holds, those whose closure holds, HasQuorum over their senders, and for the query the highest round >= 1 that
// has one.  The RoundChangeCertificate's messages are the stored rows of Answer.Record whose decision's RoundChange is 1.
func (c *Ctx) DecideRoundChangesWire(wire []byte, off []uint32, rowsCap, certsCap, rcCap int, query *RCQuery) (certs []CertVerdict, decisions []CertDecision, rows int, rc RoundChangesResult, err error) {
	n := len(off) - 1
	certs = make([]CertVerdict, certsCap+1)
	decisions = make([]CertDecision, certsCap+1)
	rc.View = make([]int32, n+1)
	rc.Stored = make([]uint64, (n+63)/64+1)
	recs := make([]RCRecord, rcCap+1)
	var answer RCAnswer
	var nRows, nCerts, nRC C.size_t
	code := C.ibft_decide_round_changes_wire(c.h, ptr8(wire), (*C.uint32_t)(unsafe.Pointer(&off[0])), C.size_t(n), C.size_t(rowsCap),
		C.size_t(certsCap), &nRows, &nCerts, (*C.ibft_cert_verdict_t)(unsafe.Pointer(&certs[0])),
		(*C.ibft_cert_decision_t)(unsafe.Pointer(&decisions[0])), nil, nil, nil, nil, nil, nil,
		(*C.ibft_rc_query_t)(unsafe.Pointer(query)), (*C.int32_t)(unsafe.Pointer(&rc.View[0])), (*C.uint64_t)(unsafe.Pointer(&rc.Stored[0])),
		(*C.ibft_rc_record_t)(unsafe.Pointer(&recs[0])), C.size_t(rcCap), &nRC, (*C.ibft_rc_answer_t)(unsafe.Pointer(&answer)))
	rc.View, rc.Stored, rc.Keys = rc.View[:n], rc.Stored[:(n+63)/64], int(nRC)
	filled := rc.Keys
	if filled > rcCap {
		filled = rcCap
	}
	if filled > n {
		filled = n
	}
	rc.Records = recs[:filled]
	if query != nil {
		rc.Answer = &answer
	}
	return certs[:int(nCerts)], decisions[:int(nCerts)], int(nRows), rc, c.check(code)
}

// WireStats reports on the context's last flat wire call (ibft_wire_stats): its rows, the rows judged through the recode class
// (FlagWireRecode; 0 without it) and the rows left WireNeedsHost.  A diagnostic: the library copies the parse results to count.
func (c *Ctx) WireStats() (rows, recoded, needsHost uint32, err error) {
	var r, d, h C.uint32_t
	rc := C.ibft_wire_stats(c.h, &r, &d, &h)
	return uint32(r), uint32(d), uint32(h), c.check(rc)
}

// CertStats reports on the context's last certificate call (ibft_cert_stats): the tree's rows, the rows that were judged (no
// pre-flag), the rows actually given to the verdict kernels, and the rows the dedup table could not place.  Without
// FlagCertDedup verdict == judged and unplaced == 0.
func (c *Ctx) CertStats() (rows, judged, verdict, unplaced uint32, err error) {
	var r, j, v, u C.uint32_t
	rc := C.ibft_cert_stats(c.h, &r, &j, &v, &u)
	return uint32(r), uint32(j), uint32(v), uint32(u), c.check(rc)
}

// CacheForm reports the table form of the device's key-cache pool (ibft_cache_form): 0 = wide (655 360 B per validator),
// 1 = glv (174 080 B per validator), and the bytes of one slot's table.  The form is the pool's, chosen by the environment
// variable IBFT_QTAB_FORM=wide|glv when the first context of the device is created; it changes no verdict.
func (c *Ctx) CacheForm() (form uint32, slotBytes uint64, err error) {
	var f C.uint32_t
	var b C.uint64_t
	rc := C.ibft_cache_form(c.h, &f, &b)
	return uint32(f), uint64(b), c.check(rc)
}

// PinnedBytes returns n bytes of page-locked memory (ibft_pinned_alloc) as a Go slice: column buffers the
// flatten step writes into once and reuses every round.  When every column of a call lies in such buffers the
// library reads them with one gather launch instead of one copy command per column.  C memory: invisible to
// the garbage collector, release with FreePinned.
func PinnedBytes(n int) []byte {
	p := C.ibft_pinned_alloc(C.size_t(n))
	if p == nil {
		return make([]byte, n) // ordinary memory works everywhere, only slower
	}
	pinnedMu.Lock()
	pinnedBlocks[uintptr(p)] = uintptr(n)
	pinnedMu.Unlock()
	return unsafe.Slice((*byte)(p), n)
}

// FreePinned releases a slice obtained from PinnedBytes (and only such a slice).
func FreePinned(b []byte) {
	if len(b) > 0 {
		pinnedMu.Lock()
		delete(pinnedBlocks, uintptr(unsafe.Pointer(&b[0])))
		pinnedMu.Unlock()
		C.ibft_pinned_free(unsafe.Pointer(&b[0]))
	}
}

// The blocks PinnedBytes handed out: C memory, which runtime.Pinner must never be given (it panics on a pointer that is
// not a Go pointer before Go 1.22).  inPinnedBytes tells whether an address lies in one of them.
var (
	pinnedMu     sync.Mutex
	pinnedBlocks = map[uintptr]uintptr{}
)

func inPinnedBytes(p unsafe.Pointer) bool {
	a := uintptr(p)
	pinnedMu.Lock()
	defer pinnedMu.Unlock()
	for base, n := range pinnedBlocks {
		if a >= base && a < base+n {
			return true
		}
	}
	return false
}

// WireRow is what the device found in one IbftMessage (ibft_wire_row_t).
type WireRow struct {
	Height, Round                            uint64
	Status, Type, PayloadKind, HasView       uint8
	HashLen, SealLen, FromLen, SigLen        uint8
	From                                     [20]byte
	ProposalHash                             [32]byte
	Recoded                                  uint8 // 1: judged through the recode class (FlagWireRecode), pad[0] of ibft_wire_row_t
	_                                        [3]byte
}

// WireNeedsHost marks a row the device did not judge (PREPREPARE / ROUND_CHANGE payloads, unknown
// fields, non-canonical encodings): decode it with proto.Unmarshal and use VerifySenders.
const WireNeedsHost = 1

// VerifySendersWire = IsValidValidator (core/ibft.go:1128) for n messages given as the bytes the
// transport delivered; wire is their concatenation, off the n+1 offsets.  Replaces proto.Unmarshal +
// PayloadNoSig (messages/proto/helper.go:12-27) + flattening for PREPARE and COMMIT messages.
func (c *Ctx) VerifySendersWire(wire []byte, off []uint32) ([]uint64, []WireRow, Tally, error) {
	n := len(off) - 1
	mask := make([]uint64, (n+63)/64+1)
	rows := make([]WireRow, n+1)
	var t C.ibft_tally_t
	rc := C.ibft_verify_senders_wire(c.h, ptr8(wire), (*C.uint32_t)(unsafe.Pointer(&off[0])), C.size_t(n),
		(*C.uint64_t)(unsafe.Pointer(&mask[0])), (*C.ibft_wire_row_t)(unsafe.Pointer(&rows[0])), &t)
	return mask, rows[:n], tally(t), c.check(rc)
}

// SetHeightSets installs the height map of VerifySendersWireSets (ibft_set_height_sets): heights in
// [firstHeight[k], firstHeight[k+1]) are judged under set rangeSet[k] of the family SetValidatorSets installed; every other
// height has no set.  firstHeight needs one entry more than rangeSet and must increase strictly; empty slices clear the map.
// SetValidatorSets DROPS the map (its indices named the old family): install it again after every family.
func (c *Ctx) SetHeightSets(firstHeight []uint64, rangeSet []uint32) error {
	if len(rangeSet) == 0 {
		return c.check(C.ibft_set_height_sets(c.h, 0, nil, nil))
	}
	if len(firstHeight) != len(rangeSet)+1 {
		return fmt.Errorf("%w: firstHeight needs one entry more than rangeSet", ErrFallback)
	}
	return c.check(C.ibft_set_height_sets(c.h, C.size_t(len(rangeSet)), (*C.uint64_t)(unsafe.Pointer(&firstHeight[0])),
		(*C.uint32_t)(unsafe.Pointer(&rangeSet[0]))))
}

// HeightSetsInfo reports the installed height map (ibft_height_sets_info): its ranges, its first mapped height and the first
// height past its last range; zeros without a map.
func (c *Ctx) HeightSetsInfo() (ranges uint32, lo, hi uint64, err error) {
	var nr C.uint32_t
	var l, h C.uint64_t
	err = c.check(C.ibft_height_sets_info(c.h, &nr, &l, &h))
	return uint32(nr), uint64(l), uint64(h), err
}

// VerifySendersWireSets = VerifySendersWire for a receive-queue batch that mixes heights (ibft_verify_senders_wire_sets): every
// message is judged under the validator set of ITS OWN height — IsValidValidator's definition (core/backend.go:41-45) — through
// the map of SetHeightSets.  set[i] is the row's set (−1: the row needs the host, has no View, or its height is in no range; such
// a row has verdict 0 and cost no signature check), vidx[i] the sender's index in that set (−1 where the bit is 0), tallies[s]
// HasQuorum over the rows of set s.  Bit for bit what SetValidators(set s) + VerifySendersWire over the rows of set s returns.
// Afterwards no batch is resident: StageWireSeals refuses.
func (c *Ctx) VerifySendersWireSets(wire []byte, off []uint32) (mask []uint64, rows []WireRow, set, vidx []int32, tallies []Tally, err error) {
	if len(off) == 0 {
		return nil, nil, nil, nil, nil, fmt.Errorf("%w: off needs n + 1 entries", ErrFallback)
	}
	n := len(off) - 1
	if len(wire) < int(off[n]) {
		return nil, nil, nil, nil, nil, fmt.Errorf("%w: wire shorter than off says", ErrFallback)
	}
	ns, _, _, err := c.ValidatorSetsInfo() // the LIBRARY's count sizes the tallies
	if err != nil {
		return nil, nil, nil, nil, nil, err
	}
	mask = make([]uint64, (n+63)/64+1)
	rows = make([]WireRow, n+1)
	set = make([]int32, n+1)
	vidx = make([]int32, n+1)
	ct := make([]C.ibft_tally_t, ns+1)
	rc := C.ibft_verify_senders_wire_sets(c.h, ptr8(wire), (*C.uint32_t)(unsafe.Pointer(&off[0])), C.size_t(n),
		(*C.uint64_t)(unsafe.Pointer(&mask[0])), (*C.ibft_wire_row_t)(unsafe.Pointer(&rows[0])),
		(*C.int32_t)(unsafe.Pointer(&set[0])), (*C.int32_t)(unsafe.Pointer(&vidx[0])), (*C.ibft_tally_t)(unsafe.Pointer(&ct[0])))
	if err = c.check(rc); err != nil {
		return nil, nil, nil, nil, nil, err
	}
	tallies = make([]Tally, ns)
	for s := range tallies {
		tallies[s] = tally(ct[s])
	}
	return mask, rows[:n], set[:n], vidx[:n], tallies, nil
}

// WireView is one quorum record of VerifySendersWireViews (ibft_wire_view_t): a (height, round, type, proposal hash) that has a
// valid message in the batch.  Tally is HasQuorum — for a PREPARE view the proposer table covers (PrepareRule) HasPrepareQuorum
// with the table's proposer — over the view's STORED rows: the messages a messages.Messages store fed the batch in row order
// still holds under this hash.
type WireView struct {
	Height, Round uint64
	Set           int32  // the set of the family the view's height is judged under
	FirstRow      uint32 // the lowest valid row of the key
	Rows          uint32 // valid rows of the view
	StoredRows    uint32 // … of them stored: the rows Tally counts
	Type          uint8  // 1 PREPARE, 2 COMMIT
	HashLen       uint8
	PrepareRule   bool
	SealRule      bool // VerifyMessagesWireViews, a COMMIT record: Tally counts only the stored rows whose committed seal verifies
	ProposalHash  [32]byte
	Tally         Tally
}

// WireViewNone and WireViewOver are the two negative values of the view column: the row is not valid / its view did not fit
// viewsCap (the row still supersedes earlier rows of its sender).
const (
	WireViewNone = int32(-1)
	WireViewOver = int32(-2)
)

// WireViewsResult is what VerifySendersWireViews returns: the five outputs of VerifySendersWireSets, byte for byte, then the
// view of every row, the stored bits (the rows a Messages store would hold after AddMessage of every valid row in row order:
// per view, a sender's later message replaces the earlier one, whatever hash it names), the records of the first viewsCap
// views and the number of views in the batch, which may exceed viewsCap.
type WireViewsResult struct {
	Mask      []uint64
	Rows      []WireRow
	Set, Vidx []int32
	Tallies   []Tally
	View      []int32
	Stored    []uint64
	Views     []WireView
	NViews    uint32
	Seal      []uint64 // VerifyMessagesWireViews only: a bit per row — the row is valid and its committed seal verifies
}

// VerifySendersWireViews = VerifySendersWireSets plus one quorum record per (height, round, type, proposal hash) that has a valid
// message in the batch (ibft_verify_senders_wire_views): what core/ibft.go:1113-1121, handlePrepare (:855-873) and handleCommit
// (:931-946) ask of GetValidMessages, for every view of a receive-queue batch in one call.  Views are numbered by their lowest
// valid row.  A PREPARE record follows HasPrepareQuorum when SetProposers covers its height and round; the proposalMessage ==
// nil case stays with the caller; the committed seals of a COMMIT record's rows are not looked at (VerifyMessagesWireViews does).  viewsCap must be positive for a batch that
// has rows; a cap above the row count behaves as the row count.
func (c *Ctx) VerifySendersWireViews(wire []byte, off []uint32, viewsCap int) (*WireViewsResult, error) {
	return c.wireViews(wire, off, viewsCap, false)
}

// VerifyMessagesWireViews = VerifySendersWireViews with the committed seals of the COMMIT rows judged in the same verdict launch
// (ibft_verify_messages_wire_views).  Seal holds a bit per row: the row is valid, sealable (a COMMIT of a member of its set
// with a 65-byte seal and a 32-byte hash) and its seal recovers to its From over the digest the seal-digest convention derives
// from the hash it names.  A COMMIT record has SealRule set and its Tally counts the stored rows whose seal bit is set —
// handleCommit's hasQuorumByMsgType (core/ibft.go:931-946) for the record of the accepted proposal's hash; the seals for
// setCommittedSeals are the rows of that view with the stored bit and the seal bit.  Everything else is VerifySendersWireViews'.
func (c *Ctx) VerifyMessagesWireViews(wire []byte, off []uint32, viewsCap int) (*WireViewsResult, error) {
	return c.wireViews(wire, off, viewsCap, true)
}

// WireSealStats reports two counts of the last VerifyMessagesWireViews (ibft_wire_seal_stats): the COMMIT rows that have a set,
// and the sealable ones — the seal checks the verdict launch was given.  0, 0 after any other wire call.
func (c *Ctx) WireSealStats() (commitRows, sealRows uint32, err error) {
	var a, b C.uint32_t
	if err = c.check(C.ibft_wire_seal_stats(c.h, &a, &b)); err != nil {
		return 0, 0, err
	}
	return uint32(a), uint32(b), nil
}

func (c *Ctx) wireViews(wire []byte, off []uint32, viewsCap int, seals bool) (*WireViewsResult, error) {
	if len(off) == 0 {
		return nil, fmt.Errorf("%w: off needs n + 1 entries", ErrFallback)
	}
	n := len(off) - 1
	if len(wire) < int(off[n]) {
		return nil, fmt.Errorf("%w: wire shorter than off says", ErrFallback)
	}
	if viewsCap < 0 || (n > 0 && viewsCap == 0) {
		return nil, fmt.Errorf("%w: viewsCap must be positive", ErrFallback)
	}
	ns, _, _, err := c.ValidatorSetsInfo() // the LIBRARY's count sizes the tallies
	if err != nil {
		return nil, err
	}
	vcap := viewsCap
	if vcap > n {
		vcap = n
	}
	r := &WireViewsResult{Mask: make([]uint64, (n+63)/64+1), Rows: make([]WireRow, n+1), Set: make([]int32, n+1), Vidx: make([]int32, n+1),
		View: make([]int32, n+1), Stored: make([]uint64, (n+63)/64+1)}
	ct := make([]C.ibft_tally_t, ns+1)
	cv := make([]C.ibft_wire_view_t, vcap+1)
	var nv C.uint32_t
	var rc C.int
	if seals {
		r.Seal = make([]uint64, (n+63)/64+1)
		rc = C.ibft_verify_messages_wire_views(c.h, ptr8(wire), (*C.uint32_t)(unsafe.Pointer(&off[0])), C.size_t(n), C.size_t(viewsCap),
			(*C.uint64_t)(unsafe.Pointer(&r.Mask[0])), (*C.ibft_wire_row_t)(unsafe.Pointer(&r.Rows[0])),
			(*C.int32_t)(unsafe.Pointer(&r.Set[0])), (*C.int32_t)(unsafe.Pointer(&r.Vidx[0])), (*C.ibft_tally_t)(unsafe.Pointer(&ct[0])),
			(*C.int32_t)(unsafe.Pointer(&r.View[0])), (*C.uint64_t)(unsafe.Pointer(&r.Stored[0])), (*C.ibft_wire_view_t)(unsafe.Pointer(&cv[0])), &nv,
			(*C.uint64_t)(unsafe.Pointer(&r.Seal[0])))
		r.Seal = r.Seal[:(n+63)/64]
	} else {
		rc = C.ibft_verify_senders_wire_views(c.h, ptr8(wire), (*C.uint32_t)(unsafe.Pointer(&off[0])), C.size_t(n), C.size_t(viewsCap),
			(*C.uint64_t)(unsafe.Pointer(&r.Mask[0])), (*C.ibft_wire_row_t)(unsafe.Pointer(&r.Rows[0])),
			(*C.int32_t)(unsafe.Pointer(&r.Set[0])), (*C.int32_t)(unsafe.Pointer(&r.Vidx[0])), (*C.ibft_tally_t)(unsafe.Pointer(&ct[0])),
			(*C.int32_t)(unsafe.Pointer(&r.View[0])), (*C.uint64_t)(unsafe.Pointer(&r.Stored[0])), (*C.ibft_wire_view_t)(unsafe.Pointer(&cv[0])), &nv)
	}
	if err = c.check(rc); err != nil {
		return nil, err
	}
	r.Rows, r.Set, r.Vidx, r.View = r.Rows[:n], r.Set[:n], r.Vidx[:n], r.View[:n]
	r.Mask, r.Stored = r.Mask[:(n+63)/64], r.Stored[:(n+63)/64]
	r.Tallies = make([]Tally, ns)
	for s := range r.Tallies {
		r.Tallies[s] = tally(ct[s])
	}
	r.NViews = uint32(nv)
	filled := int(r.NViews)
	if filled > vcap {
		filled = vcap
	}
	r.Views = make([]WireView, filled)
	for v := range r.Views {
		w := cv[v]
		o := &r.Views[v]
		o.Height, o.Round, o.Set = uint64(w.height), uint64(w.round), int32(w.set)
		o.FirstRow, o.Rows, o.StoredRows = uint32(w.first_row), uint32(w.rows), uint32(w.stored_rows)
		o.Type, o.HashLen, o.PrepareRule = uint8(w._type), uint8(w.hash_len), w.prepare_rule != 0
		o.SealRule = w.pad[C.IBFT_WIRE_VIEW_SEAL_RULE] != 0
		for i := range o.ProposalHash {
			o.ProposalHash[i] = byte(w.proposal_hash[i])
		}
		o.Tally = tally(w.tally)
	}
	return r, nil
}

// StageWireSeals makes the COMMIT seals found by the last VerifySendersWire the resident seal batch;
// follow with SealsRun (IsValidCommittedSeal without a second upload).
func (c *Ctx) StageWireSeals() error { return c.check(C.ibft_wire_stage_seals(c.h)) }

// sealRows asks the LIBRARY how many rows the resident batch and the oldest submitted pass have (ibft_seals_rows): verdict
// buffers are sized from these, never from a count the caller passes along — a count that is too small would let C write
// past the Go slice (ADVICE round 5).
func (c *Ctx) sealRows() (resident, oldest int, err error) {
	var a, b C.uint32_t
	if err = c.check(C.ibft_seals_rows(c.h, &a, &b)); err != nil {
		return 0, 0, err
	}
	return int(a), int(b), nil
}

// PipelineStats = how many submitted passes had their tally on the side stream (next to the following pass's verdict kernel,
// DESIGN.md §5.10) and how many batches of 65 537 … 98 304 rows went out as two launches, since the context was created.
func (c *Ctx) PipelineStats() (sideTallies, splitBatches int, err error) {
	var a, b C.uint32_t
	if err = c.check(C.ibft_pipeline_stats(c.h, &a, &b)); err != nil {
		return 0, 0, err
	}
	return int(a), int(b), nil
}

// AltVerdictPasses reports how many submitted passes put their verdict launch on the second verdict stream
// (ibft_pipeline_stats_ex; IBFT_ALT_VERDICT, DESIGN.md §5.10), since the context was created.
func (c *Ctx) AltVerdictPasses() (int, error) {
	var a C.uint32_t
	if err := c.check(C.ibft_pipeline_stats_ex(c.h, nil, nil, &a)); err != nil {
		return 0, err
	}
	return int(a), nil
}

// SealsRows = rows of the resident seal batch as the library counts them.
func (c *Ctx) SealsRows() (int, error) {
	n, _, err := c.sealRows()
	return n, err
}

// SealsRun = one pass of IsValidCommittedSeal + HasQuorum over the RESIDENT seal batch
// (ibft_seals_run: launch + fetch); the mask has a word per 64 resident rows (SealsRows).
func (c *Ctx) SealsRun() ([]uint64, Tally, error) {
	n, _, err := c.sealRows()
	if err != nil {
		return nil, Tally{}, err
	}
	mask := make([]uint64, (n+63)/64+1)
	var t C.ibft_tally_t
	rc := C.ibft_seals_run(c.h, (*C.uint64_t)(unsafe.Pointer(&mask[0])), &t)
	return mask, tally(t), c.check(rc)
}

// SealsStageNext copies the NEXT seal batch into the context's spare column set on a copy stream of its own while the
// kernels of the resident batch run; SealsSwap makes it the resident batch.  Per step of a sustained stream of COMMIT
// sets (one GetValidMessages walk per wake-up, core/ibft.go:931-946): SealsLaunch(k) → SealsStageNext(k+1) →
// SealsFetch(k) → SealsSwap.  Every column must hold exactly n = len(sig65)/65 rows (ErrFallback otherwise: the copy would
// read past a slice); preFlags may be nil.  The copy is asynchronous — the library reads the slices after this call has
// returned — so they are pinned here until SealsSwap (cgo's pointer rule; the caller must not write to them before
// either).  Slices carved from PinnedBytes are page-locked as well, and only then does the copy overlap the kernels.
func (c *Ctx) SealsStageNext(hash32, sig65, signer20, preFlags []byte) error {
	n := len(sig65) / 65
	if n == 0 || len(sig65) != 65*n || len(hash32) != 32*n || len(signer20) != 20*n || (preFlags != nil && len(preFlags) != n) {
		return ErrFallback
	}
	c.next.Unpin() // (a batch staged and never swapped in is replaced: the library restarts the copy)
	c.next.Pin(&hash32[0])
	c.next.Pin(&sig65[0])
	c.next.Pin(&signer20[0])
	if preFlags != nil {
		c.next.Pin(&preFlags[0])
	}
	err := c.check(C.ibft_seals_stage_next(c.h, ptr8(hash32), ptr8(sig65), ptr8(signer20), ptr8(preFlags), C.size_t(n)))
	if err != nil {
		c.next.Unpin()
	}
	return err
}

// SealsSubmit enqueues one more pass over the resident seal batch and returns at once (at most two in flight);
// SealsCollect waits for the OLDEST submitted pass only and returns its verdict words and tally.  Keeping one pass in flight
// lets the device run back to back while Go handles the previous pass's result (ibft_seals_submit / ibft_seals_collect).
func (c *Ctx) SealsSubmit() error { return c.check(C.ibft_seals_submit(c.h)) }

// SealsCollect: see SealsSubmit.  The mask is sized for the rows of THAT pass as the library recorded them at submit time
// (a SealsSwap to a batch of another size may have come in between); rows = that count.
func (c *Ctx) SealsCollect() (mask []uint64, rows int, t Tally, err error) {
	_, rows, err = c.sealRows()
	if err != nil {
		return nil, 0, Tally{}, err
	}
	if rows == 0 {
		return nil, 0, Tally{}, ErrFallback // nothing submitted
	}
	mask = make([]uint64, (rows+63)/64+1)
	var ct C.ibft_tally_t
	rc := C.ibft_seals_collect(c.h, (*C.uint64_t)(unsafe.Pointer(&mask[0])), &ct)
	return mask, rows, tally(ct), c.check(rc)
}

// SealsSwap: see SealsStageNext.  Waits for the copy of the staged batch, after which its Go slices are released.
func (c *Ctx) SealsSwap() error {
	err := c.check(C.ibft_seals_swap(c.h, 1))
	c.next.Unpin()
	return err
}

// IssueProbe = the device canary (ibft_issue_probe): wall nanoseconds per aligned 8-byte VALU instruction per SIMD at one
// wavefront per SIMD — 1.89 on a healthy MI355X; a Backend logs it at start-up.
func (c *Ctx) IssueProbe() (nsPerInst float32, err error) {
	var ns, ms C.float
	err = c.check(C.ibft_issue_probe(c.h, &ns, &ms))
	return float32(ns), err
}

// SignSeals = n × Backend.BuildCommitMessage's committed seal (core/backend.go:12-34) for a SIMULATOR that plays
// n validators in one process: sk and hashes are n×32 bytes; returns the n×65 seals, the n×20 signer addresses
// and ok[i] == 0 for a key outside [1, n).  Leaves the batch resident: SealsRun() verifies it without an upload.
// Not for a production validator's key (include/ibftgpu.h, ibft_sign_seals).
func (c *Ctx) SignSeals(sk, hashes []byte) (seals, signers, ok []byte, err error) {
	n := len(sk) / 32
	if n == 0 || len(hashes) != 32*n {
		return nil, nil, nil, ErrFallback
	}
	seals, signers, ok = make([]byte, 65*n), make([]byte, 20*n), make([]byte, n)
	rc := C.ibft_sign_seals(c.h, (*C.uint8_t)(unsafe.Pointer(&sk[0])), (*C.uint8_t)(unsafe.Pointer(&hashes[0])),
		C.size_t(n), (*C.uint8_t)(unsafe.Pointer(&seals[0])), (*C.uint8_t)(unsafe.Pointer(&signers[0])),
		(*C.uint8_t)(unsafe.Pointer(&ok[0])))
	return seals, signers, ok, c.check(rc)
}

// Nonce rules of SignSealsNonce (IBFT_SIGN_NONCE_*).
const (
	SignNonceKeccak  uint32 = C.IBFT_SIGN_NONCE_KECCAK  // SignSeals' rule: keccak256(sk ‖ digest ‖ ctr) mod n
	SignNonceRFC6979 uint32 = C.IBFT_SIGN_NONCE_RFC6979 // RFC 6979 §3.2, HMAC-SHA-256, bits2octets(h1) = h1 mod n (btcec's seals)
)

// SignSealsNonce = SignSeals under a chosen nonce rule (ibft_sign_seals_ex): with SignNonceRFC6979 the seals are the ones
// btcec / bitcoinjs produce for the same key and digest, so a rig can compare simulated validators with real ones.
// Everything SignSeals says holds; an unknown rule is refused (the error names it).
func (c *Ctx) SignSealsNonce(sk, hashes []byte, nonce uint32) (seals, signers, ok []byte, err error) {
	n := len(sk) / 32
	if n == 0 || len(hashes) != 32*n {
		return nil, nil, nil, ErrFallback
	}
	seals, signers, ok = make([]byte, 65*n), make([]byte, 20*n), make([]byte, n)
	rc := C.ibft_sign_seals_ex(c.h, (*C.uint8_t)(unsafe.Pointer(&sk[0])), (*C.uint8_t)(unsafe.Pointer(&hashes[0])),
		C.size_t(n), C.uint32_t(nonce), (*C.uint8_t)(unsafe.Pointer(&seals[0])), (*C.uint8_t)(unsafe.Pointer(&signers[0])),
		(*C.uint8_t)(unsafe.Pointer(&ok[0])))
	return seals, signers, ok, c.check(rc)
}

// SignMessages = n × Backend.BuildPrepareMessage / BuildCommitMessage (core/backend.go:12-34) for a SIMULATOR
// (ibft_sign_messages_wire): row i is (sk[32i:], types[i] = 1 PREPARE / 2 COMMIT, heights[i], rounds[i], hashes[32i:]) and
// comes back as the wire bytes of its message, wire[off[i]:off[i+1]] — the form VerifySendersWire reads —, with the sender
// addresses (n×20) and ok[i] == 0 for a key outside [1, n) (a row of its normal length with a zero From, signature and seal).
// Leaves no batch resident.  Not for a production validator's key (include/ibftgpu.h, ibft_sign_seals).
func (c *Ctx) SignMessages(sk, types []byte, heights, rounds []uint64, hashes []byte, nonce uint32) (wire []byte, off []uint32, from, ok []byte, err error) {
	n := len(types)
	if n == 0 || len(sk) != 32*n || len(heights) != n || len(rounds) != n || len(hashes) != 32*n {
		return nil, nil, nil, nil, ErrFallback
	}
	wire, off, from, ok = make([]byte, int(C.IBFT_SIGN_MESSAGE_MAX)*n), make([]uint32, n+1), make([]byte, 20*n), make([]byte, n)
	rc := C.ibft_sign_messages_wire(c.h, (*C.uint8_t)(unsafe.Pointer(&sk[0])), (*C.uint8_t)(unsafe.Pointer(&types[0])),
		(*C.uint64_t)(unsafe.Pointer(&heights[0])), (*C.uint64_t)(unsafe.Pointer(&rounds[0])),
		(*C.uint8_t)(unsafe.Pointer(&hashes[0])), C.size_t(n), C.uint32_t(nonce), (*C.uint8_t)(unsafe.Pointer(&wire[0])),
		C.size_t(len(wire)), (*C.uint32_t)(unsafe.Pointer(&off[0])), (*C.uint8_t)(unsafe.Pointer(&from[0])),
		(*C.uint8_t)(unsafe.Pointer(&ok[0])))
	if err = c.check(rc); err != nil {
		return nil, nil, nil, nil, err
	}
	return wire[:off[n]], off, from, ok, nil
}

// SignEnvelopes = n × Backend.BuildPrePrepareMessage / BuildRoundChangeMessage (core/backend.go:12-34) for a SIMULATOR
// (ibft_sign_envelopes_wire): row i is (sk[32i:], types[i] = 0 PREPREPARE / 3 ROUND_CHANGE, heights[i], rounds[i], the encoded
// PrePrepareMessage / RoundChangeMessage body[bodyAt[i]:bodyAt[i]+bodyLen[i]]) — rows may name the same or overlapping ranges, a
// certificate many senders carry is passed once — and comes back as the wire bytes of its message, wire[off[i]:off[i+1]] — the
// form VerifyCertificatesWire reads —, with the sender addresses (n×20) and ok[i] == 0 for a key outside [1, n) (a row of its
// normal length with a zero From and signature around its body).  Leaves no batch resident.  Not for a production validator's
// key (include/ibftgpu.h, ibft_sign_seals).
func (c *Ctx) SignEnvelopes(sk, types []byte, heights, rounds []uint64, body []byte, bodyAt, bodyLen []uint32, nonce uint32) (wire []byte, off []uint32, from, ok []byte, err error) {
	n := len(types)
	if n == 0 || len(sk) != 32*n || len(heights) != n || len(rounds) != n || len(bodyAt) != n || len(bodyLen) != n {
		return nil, nil, nil, nil, ErrFallback
	}
	total := 0
	for _, l := range bodyLen {
		total += 121 + int(l) // the head in front of a body is at most 121 bytes
	}
	var bp *C.uint8_t
	if len(body) > 0 {
		bp = (*C.uint8_t)(unsafe.Pointer(&body[0]))
	}
	wire, off, from, ok = make([]byte, total), make([]uint32, n+1), make([]byte, 20*n), make([]byte, n)
	rc := C.ibft_sign_envelopes_wire(c.h, (*C.uint8_t)(unsafe.Pointer(&sk[0])), (*C.uint8_t)(unsafe.Pointer(&types[0])),
		(*C.uint64_t)(unsafe.Pointer(&heights[0])), (*C.uint64_t)(unsafe.Pointer(&rounds[0])), bp, C.size_t(len(body)),
		(*C.uint32_t)(unsafe.Pointer(&bodyAt[0])), (*C.uint32_t)(unsafe.Pointer(&bodyLen[0])), C.size_t(n), C.uint32_t(nonce),
		(*C.uint8_t)(unsafe.Pointer(&wire[0])), C.size_t(len(wire)), (*C.uint32_t)(unsafe.Pointer(&off[0])),
		(*C.uint8_t)(unsafe.Pointer(&from[0])), (*C.uint8_t)(unsafe.Pointer(&ok[0])))
	if err = c.check(rc); err != nil {
		return nil, nil, nil, nil, err
	}
	return wire[:off[n]], off, from, ok, nil
}

// Group is one process driving several MI355X (ibft_group_*): the rows of a batch are sharded over the
// devices in 64-aligned ranges and ONE RCCL all-reduce inside the library merges the verdict words and the
// ranks' distinct-sender bitmaps (a validator with valid rows in two shards is counted once, as HasQuorum's
// address set does) — for validator sets beyond a single GPU's batch (BASELINE configs #4 / #5).
type Group struct{ g *C.ibft_group }

func NewGroup(devices []int32, o Options) (*Group, error) {
	var flags C.uint32_t
	if o.StrictLowS {
		flags |= C.IBFT_FLAG_STRICT_LOW_S
	}
	if o.KeyCache {
		flags |= C.IBFT_FLAG_PUBKEY_CACHE
	}
	if o.CertDedup {
		flags |= C.IBFT_FLAG_CERT_DEDUP
	}
	if o.WireRecode {
		flags |= C.IBFT_FLAG_WIRE_RECODE
	}
	var g *C.ibft_group
	rc := C.ibft_group_create((*C.int32_t)(unsafe.Pointer(&devices[0])), C.uint32_t(len(devices)), flags,
		C.uint32_t(o.MaxRows), &g)
	if rc != C.IBFT_OK {
		return nil, fmt.Errorf("%w: %s", ErrFallback, C.GoString(C.ibft_strerror(rc)))
	}
	gr := &Group{g: g}
	runtime.SetFinalizer(gr, (*Group).Close)
	return gr, nil
}

func (g *Group) Close() {
	if g.g != nil {
		C.ibft_group_destroy(g.g)
		g.g = nil
	}
}

func (g *Group) SetValidators(height uint64, addrs20 []byte, power []uint64) error {
	var pp *C.uint64_t
	if len(power) > 0 {
		pp = (*C.uint64_t)(unsafe.Pointer(&power[0]))
	}
	if rc := C.ibft_group_set_validators(g.g, C.uint64_t(height), ptr8(addrs20), pp, C.size_t(len(power))); rc != C.IBFT_OK {
		return fmt.Errorf("%w: %s", ErrFallback, C.GoString(C.ibft_strerror(rc)))
	}
	return nil
}

// VerifySeals = IsValidCommittedSeal + HasQuorum over n rows sharded across the group's devices; mask and
// tally are the merged (global) ones.
func (g *Group) VerifySeals(hash32, sig65, signer20, preFlags []byte) ([]uint64, Tally, error) {
	n := len(sig65) / 65
	mask := make([]uint64, (n+63)/64+1)
	var t C.ibft_tally_t
	rc := C.ibft_group_verify_seals(g.g, ptr8(hash32), ptr8(sig65), ptr8(signer20), ptr8(preFlags), C.size_t(n),
		(*C.uint64_t)(unsafe.Pointer(&mask[0])), &t)
	if rc != C.IBFT_OK {
		return nil, Tally{}, fmt.Errorf("%w: %s", ErrFallback, C.GoString(C.ibft_strerror(rc)))
	}
	return mask, tally(t), nil
}

// VerifySenders = IsValidValidator + HasQuorum, sharded like VerifySeals (payload/off: concatenated
// PayloadNoSig bytes and their n+1 offsets).
func (g *Group) VerifySenders(payload []byte, off []uint32, sig65, from20, preFlags []byte) ([]uint64, Tally, error) {
	n := len(sig65) / 65
	mask := make([]uint64, (n+63)/64+1)
	var t C.ibft_tally_t
	rc := C.ibft_group_verify_senders(g.g, ptr8(payload), (*C.uint32_t)(unsafe.Pointer(&off[0])), ptr8(sig65),
		ptr8(from20), ptr8(preFlags), C.size_t(n), (*C.uint64_t)(unsafe.Pointer(&mask[0])), &t)
	if rc != C.IBFT_OK {
		return nil, Tally{}, fmt.Errorf("%w: %s", ErrFallback, C.GoString(C.ibft_strerror(rc)))
	}
	return mask, tally(t), nil
}

// VerifyMessages judges a whole PREPARE / COMMIT set sharded by message (Ctx.VerifyMessages' columns and
// results; seal65 nil for a PREPARE set; digest32 nil to have raw ‖ BE64(round) hashed on the devices).
func (g *Group) VerifyMessages(payload []byte, off []uint32, msgSig65, from20, hash32, hashLen, seal65,
	senderPre, validPre, raw []byte, round uint64, digest32, proposer20 []byte) (senders, valid []uint64, t Tally, err error) {
	n := len(msgSig65) / 65
	senders = make([]uint64, (n+63)/64+1)
	valid = make([]uint64, (n+63)/64+1)
	var ct C.ibft_tally_t
	rc := C.ibft_group_verify_messages(g.g, ptr8(payload), (*C.uint32_t)(unsafe.Pointer(&off[0])), ptr8(msgSig65),
		ptr8(from20), ptr8(hash32), ptr8(hashLen), ptr8(seal65), ptr8(senderPre), ptr8(validPre), C.size_t(n),
		ptr8(raw), C.size_t(len(raw)), C.uint64_t(round), ptr8(digest32), ptr8(proposer20),
		(*C.uint64_t)(unsafe.Pointer(&senders[0])), (*C.uint64_t)(unsafe.Pointer(&valid[0])), &ct)
	if rc != C.IBFT_OK {
		return nil, nil, Tally{}, fmt.Errorf("%w: %s", ErrFallback, C.GoString(C.ibft_strerror(rc)))
	}
	return senders, valid, tally(ct), nil
}

// VerifyCertificatesWire judges the certificate trees of raw PREPREPARE / ROUND_CHANGE messages sharded by carrier over the
// group's devices (Ctx.VerifyCertificatesWire's arguments and results; the rows are numbered as one call over all messages
// numbers them).  No tally is taken and the devices exchange nothing.
func (g *Group) VerifyCertificatesWire(wire []byte, off []uint32, rowsCap int) (nodes []CertNode, class []byte, sender, hash, self []uint64, err error) {
	n := len(off) - 1
	nodes = make([]CertNode, rowsCap+1)
	class = make([]byte, rowsCap+1)
	sender, hash, self = make([]uint64, (rowsCap+63)/64+1), make([]uint64, (rowsCap+63)/64+1), make([]uint64, (rowsCap+63)/64+1)
	var rows C.size_t
	rc := C.ibft_group_verify_certificates_wire(g.g, ptr8(wire), (*C.uint32_t)(unsafe.Pointer(&off[0])), C.size_t(n), C.size_t(rowsCap), &rows,
		(*C.ibft_cert_node_t)(unsafe.Pointer(&nodes[0])), nil, ptr8(class), (*C.uint64_t)(unsafe.Pointer(&sender[0])),
		(*C.uint64_t)(unsafe.Pointer(&hash[0])), (*C.uint64_t)(unsafe.Pointer(&self[0])))
	if rc != C.IBFT_OK {
		return nil, nil, nil, nil, nil, fmt.Errorf("%w: %s", ErrFallback, C.GoString(C.ibft_strerror(rc)))
	}
	return nodes[:int(rows)], class[:int(rows)], sender, hash, self, nil
}

func tally(t C.ibft_tally_t) Tally {
	return Tally{uint64(t.quorum_lo), uint64(t.quorum_hi), uint64(t.power_lo), uint64(t.power_hi),
		uint32(t.valid_rows), uint32(t.distinct_senders), t.has_quorum != 0, uint32(t.shard_overlap), uint32(t.proposer_rows)}
}

// Bit reports row i's verdict.
func Bit(mask []uint64, i int) bool { return mask[i>>6]>>(uint(i)&63)&1 == 1 }
