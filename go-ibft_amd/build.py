"""Build libibftgpu.so for gfx950 with hipcc (in-tree, so it travels with gpurun)."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libibftgpu.so")
SOURCES = ["ibftgpu.hip", "kernels.hip.h", "recover_dev.h", "verify_dev.h", "wave_fe_dev.h", "wire_dev.h", "wire_recode_dev.h", "wire_sets_dev.h", "tally_dev.h", "wire_views_dev.h", "wire_seals_dev.h", "round_change_dev.h", "cert_wave_dev.h", "cert_scan_dev.h", "cert_verdict_dev.h", "cert_decide_dev.h", "cert_dedup_dev.h", "cert_dedup_kernels.h", "modinv_dev.h",
           "sign_dev.h", "sign_message_dev.h", "sign_envelope_dev.h", "sha256_dev.h", "secp256k1_dev.h", "keccak_dev.h", "keccak_row_dev.h", os.path.join("..", "..", "include", "ibftgpu.h")]
# Code-generation flags of the product library (part of its build stamp).  max-ilp: the verdict kernels run ONE wavefront per
# SIMD at the sizes that matter (N ≤ 4 096), where every hazard s_nop is a lost issue slot — scheduling for instruction-level
# parallelism instead of register pressure takes the s_nops of ecrecover_rows_kernel from 399 to 114 (133 → 174 VGPRs, still
# two wavefronts per SIMD) and the kernels 3–4.6 % down at N = 64 … 4 096, nothing lost at 16 384 / 65 536
# (profiles/r03r_*).  IBFT_HIPCC_FLAGS adds to them for experiments, IBFT_NO_CODEGEN_FLAGS=1 drops them (the A/B of
# profiles/r03r_sched_ab.txt).
CODEGEN_FLAGS = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
EXTRA_FLAGS = ([] if os.environ.get("IBFT_NO_CODEGEN_FLAGS") == "1" else CODEGEN_FLAGS) + os.environ.get("IBFT_HIPCC_FLAGS", "").split()
HOST_HARNESS = os.path.join(CSRC, "libdev_arith_host.so")
WAVE_HARNESS = os.path.join(CSRC, "libdev_wave_host.so")
CERT_WAVE_HARNESS = os.path.join(CSRC, "libdev_cert_wave_host.so")


def _digest(deps: list[str], extra: str = "") -> str:
    import hashlib
    h = hashlib.sha256(extra.encode())
    for d in deps:
        with open(os.path.join(CSRC, d), "rb") as f:
            h.update(d.encode() + b"\0" + f.read() + b"\0")
    return h.hexdigest()


def _file_sha256(path: str) -> str:
    import hashlib
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def _read_stamp(target: str) -> list[str]:
    try:
        with open(target + ".stamp") as f:
            return f.read().split("\n")
    except OSError:
        return []


def _stale(target: str, deps: list[str], extra: str = "") -> bool:
    """A target is current when (1) the digest of its sources (+ the compile command) equals the one recorded next to it
    when it was built — modification times say nothing after a checkout or a copy to another box — and (2) the target's OWN
    sha256 equals the one recorded: a binary that something rewrote after the build (round-4 review: objcopy, in place) is
    rebuilt, never shipped."""
    st = _read_stamp(target)
    if not os.path.exists(target) or len(st) < 2:
        return True
    return st[0].strip() != _digest(deps, extra) or st[1].strip() != _file_sha256(target)


def _mark(target: str, deps: list[str], extra: str = "", flavour: str = "") -> None:
    """stamp = source digest, the built file's sha256, how it was built (line 3: what bench.py / build_info() report)"""
    with open(target + ".stamp", "w") as f:
        f.write(_digest(deps, extra) + "\n" + _file_sha256(target) + "\n" + flavour + "\n")


def build_info(target: str | None = None) -> dict:
    """what the stamp says about a built target: {"flavour": "phase_align" | "phase_align_failed: …" | "one_step", "sha256": …,
    "intact": the file still is what the build wrote}"""
    target = target or LIB
    st = _read_stamp(target)
    if len(st) < 3 or not os.path.exists(target):
        return {"flavour": None, "sha256": None, "intact": False}
    return {"flavour": st[2].strip(), "sha256": st[1].strip(), "intact": st[1].strip() == _file_sha256(target)}


LLVM_BIN = "/opt/rocm/lib/llvm/bin"
PHASE_ALIGN = os.environ.get("IBFT_NO_PHASE_ALIGN") != "1"


def _build_lib_phase_aligned(verbose: bool) -> None:
    """hipcc's own steps, taken apart so that the device assembly passes through go-ibft_amd/phase_align.py (8-byte
    instructions on 8-byte boundaries: profiles/r04o_*): device code → assembly → aligned assembly → code object →
    fat binary → host compile with that fat binary embedded → libibftgpu.so."""
    import tempfile
    try:
        from . import phase_align
    except ImportError:  # (run as a script: python go-ibft_amd/build.py)
        import importlib.util
        spec = importlib.util.spec_from_file_location("phase_align", os.path.join(HERE, "phase_align.py"))
        phase_align = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(phase_align)
    src = os.path.join(CSRC, "ibftgpu.hip")
    common = ["--offload-arch=gfx950", "-O3", "-std=c++17", *EXTRA_FLAGS]
    with tempfile.TemporaryDirectory(prefix="ibftgpu_build_") as d:
        dev_s, al_s, dev_o, dev_out, fb = (os.path.join(d, n) for n in ("dev.s", "dev.aligned.s", "dev.o", "dev.out", "dev.hipfb"))
        def run(cmd):   # stderr is kept: a failing sub-step must say why
            p = subprocess.run(cmd, cwd=CSRC, stderr=subprocess.PIPE, text=True)
            if verbose and p.stderr:
                print(p.stderr, end="", flush=True)
            if p.returncode != 0:
                raise RuntimeError(f"{os.path.basename(cmd[0])} returned {p.returncode}: {p.stderr[-2000:]}")
        run(["hipcc", *common, "--cuda-device-only", "-S", "-o", dev_s, src])
        phase_align.align_file(dev_s, al_s, dev_o, verbose=verbose)
        run([os.path.join(LLVM_BIN, "lld"), "-flavor", "gnu", "-m", "elf64_amdgpu", "--no-undefined", "-shared", "-o", dev_out, dev_o])
        run([os.path.join(LLVM_BIN, "clang-offload-bundler"), "-type=o", "-bundle-align=4096",
             "-targets=host-x86_64-unknown-linux-gnu,hipv4-amdgcn-amd-amdhsa--gfx950", "-input=/dev/null", f"-input={dev_out}", f"-output={fb}"])
        run(["hipcc", *common, "--cuda-host-only", "-Xclang", "-fcuda-include-gpubinary", "-Xclang", fb, "-shared", "-fPIC",
             "-o", LIB, src, "-ldl"])


def build_lib(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", *EXTRA_FLAGS, "-shared", "-fPIC",
           "-o", LIB, os.path.join(CSRC, "ibftgpu.hip"), "-ldl"]
    stamp_extra = " ".join(cmd[:-3]) + (" +phase_align" if PHASE_ALIGN else "")
    deps = SOURCES + ([os.path.join("..", "phase_align.py")] if PHASE_ALIGN else [])
    # a stamp that records a FAILED alignment step is retried (the fallback library is the same code without the step)
    retry = PHASE_ALIGN and (build_info(LIB)["flavour"] or "").startswith("phase_align_failed")
    if force or retry or _stale(LIB, deps, stamp_extra):
        done = False
        flavour = "one_step"
        if PHASE_ALIGN:
            try:
                if verbose:
                    print(" ".join(cmd), "  (+ phase_align.py between device assembly and code object)", flush=True)
                _build_lib_phase_aligned(verbose)
                done = True
                flavour = "phase_align"
            except Exception as e:  # the one-shot build below is the same library without the alignment step
                print(f"build: phase-aligned build failed ({e}); building with hipcc in one step", flush=True)
                flavour = "phase_align_failed: " + " ".join(str(e).split())[:300]
        if not done:
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd, cwd=CSRC)
        _mark(LIB, deps, stamp_extra, flavour)
    return LIB


DEVTEST = os.path.join(CSRC, "libibft_devtest.so")


def build_devtest(force: bool = False) -> str:
    """TEST-ONLY: single arithmetic primitives (tests/test_gpu_arith.py), the certificate tree's level scans
    (tests/test_gpu_cert_scan.py) and its dedup kernels (tests/test_gpu_cert_dedup_kernels.py) as gfx950 kernels."""
    deps = ["devtest.hip", "recover_dev.h", "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h", "keccak_row_dev.h", "wave_fe_dev.h", "verify_dev.h",
            "sign_dev.h", "sha256_dev.h", "cert_scan_dev.h", "wire_dev.h", "cert_dedup_dev.h", "cert_dedup_kernels.h"]
    if force or _stale(DEVTEST, deps):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-w",
                               "-o", DEVTEST, os.path.join(CSRC, "devtest.hip")], cwd=CSRC)
        _mark(DEVTEST, deps)
    return DEVTEST


def build_host_harness(force: bool = False) -> str:
    """TEST-ONLY: the device arithmetic headers compiled for the CPU (hipcc host pass)."""
    deps = ["host_arith_harness.hip", "sign_dev.h", "sha256_dev.h", "recover_dev.h", "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h", "wire_dev.h", "verify_dev.h"]
    if force or _stale(HOST_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", HOST_HARNESS, os.path.join(CSRC, "host_arith_harness.hip")], cwd=CSRC)
        _mark(HOST_HARNESS, deps)
    return HOST_HARNESS


def build_wave_harness(force: bool = False) -> str:
    """TEST-ONLY: wave_fe_dev.h (one wavefront per signature) on the CPU through wave_emul.h."""
    deps = ["host_wave_harness.hip", "wave_fe_dev.h", "wave_emul.h", "recover_dev.h", "verify_dev.h",
            "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h", "keccak_row_dev.h"]
    if force or _stale(WAVE_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", WAVE_HARNESS, os.path.join(CSRC, "host_wave_harness.hip")], cwd=CSRC)
        _mark(WAVE_HARNESS, deps)
    return WAVE_HARNESS


def build_cert_wave_harness(force: bool = False) -> str:
    """TEST-ONLY: cert_wave_dev.h (Keccak by one wavefront, the certificate walk) on the CPU through wave_emul.h."""
    deps = ["host_cert_wave_harness.hip", "cert_wave_dev.h", "wave_emul.h", "wire_dev.h", "keccak_dev.h"]
    if force or _stale(CERT_WAVE_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", CERT_WAVE_HARNESS, os.path.join(CSRC, "host_cert_wave_harness.hip")], cwd=CSRC)
        _mark(CERT_WAVE_HARNESS, deps)
    return CERT_WAVE_HARNESS


ROW_KECCAK_HARNESS = os.path.join(CSRC, "libdev_row_keccak_host.so")


def build_row_keccak_harness(force: bool = False) -> str:
    """TEST-ONLY: keccak_row_dev.h (the address hash with its state spread over a row's lanes) on the CPU through wave_emul.h."""
    deps = ["host_row_keccak_harness.hip", "keccak_row_dev.h", "wave_fe_dev.h", "wave_emul.h", "recover_dev.h", "verify_dev.h",
            "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h"]
    if force or _stale(ROW_KECCAK_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", ROW_KECCAK_HARNESS, os.path.join(CSRC, "host_row_keccak_harness.hip")], cwd=CSRC)
        _mark(ROW_KECCAK_HARNESS, deps)
    return ROW_KECCAK_HARNESS


ROW_SCALARS_HARNESS = os.path.join(CSRC, "libdev_row_scalars_host.so")


def build_row_scalars_harness(force: bool = False) -> str:
    """TEST-ONLY: wv::row_scalars (the scalar stage of the row forms, one multiplication for both halves of a row) on the CPU through wave_emul.h."""
    deps = ["host_row_scalars_harness.hip", "wave_fe_dev.h", "wave_emul.h", "recover_dev.h", "verify_dev.h",
            "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h", "keccak_row_dev.h"]
    if force or _stale(ROW_SCALARS_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", ROW_SCALARS_HARNESS, os.path.join(CSRC, "host_row_scalars_harness.hip")], cwd=CSRC)
        _mark(ROW_SCALARS_HARNESS, deps)
    return ROW_SCALARS_HARNESS


PROPOSAL_DIGEST_HARNESS = os.path.join(CSRC, "libdev_proposal_digest_host.so")


def build_proposal_digest_harness(force: bool = False) -> str:
    """TEST-ONLY: the lane and the wavefront form of proposal_digest_kernel's absorb routine on the CPU."""
    deps = ["host_proposal_digest_harness.hip", "cert_wave_dev.h", "wave_emul.h", "wire_dev.h", "keccak_dev.h"]
    if force or _stale(PROPOSAL_DIGEST_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", PROPOSAL_DIGEST_HARNESS, os.path.join(CSRC, "host_proposal_digest_harness.hip")], cwd=CSRC)
        _mark(PROPOSAL_DIGEST_HARNESS, deps)
    return PROPOSAL_DIGEST_HARNESS


BLOCK_SETS_HARNESS = os.path.join(CSRC, "libdev_block_sets_host.so")


def build_block_sets_harness(force: bool = False) -> str:
    """TEST-ONLY: the per-row decision of block_tally_kernel under a family of sets (recover_dev.h: valsets_*) on the CPU."""
    deps = ["host_block_sets_harness.hip", "recover_dev.h", "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h"]
    if force or _stale(BLOCK_SETS_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", BLOCK_SETS_HARNESS, os.path.join(CSRC, "host_block_sets_harness.hip")], cwd=CSRC)
        _mark(BLOCK_SETS_HARNESS, deps)
    return BLOCK_SETS_HARNESS


BLOCK_HEAD_HARNESS = os.path.join(CSRC, "libdev_block_head_host.so")


def build_block_head_harness(force: bool = False) -> str:
    """TEST-ONLY: the per-row body of block_head_kernel (recover_dev.h: block_of_row, block_head_row) on the CPU."""
    deps = ["host_block_head_harness.hip", "recover_dev.h", "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h"]
    if force or _stale(BLOCK_HEAD_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", BLOCK_HEAD_HARNESS, os.path.join(CSRC, "host_block_head_harness.hip")], cwd=CSRC)
        _mark(BLOCK_HEAD_HARNESS, deps)
    return BLOCK_HEAD_HARNESS


SIGN_NONCE_HARNESS = os.path.join(CSRC, "libdev_sign_nonce_host.so")


def build_sign_nonce_harness(force: bool = False) -> str:
    """TEST-ONLY: sha256_dev.h and the RFC 6979 nonce rule of sign_dev.h (compression, HMAC, the DRBG, the signing row) on the CPU."""
    deps = ["host_sign_nonce_harness.hip", "host_gtab.h", "sign_dev.h", "sha256_dev.h", "recover_dev.h", "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h"]
    if force or _stale(SIGN_NONCE_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", SIGN_NONCE_HARNESS, os.path.join(CSRC, "host_sign_nonce_harness.hip")], cwd=CSRC)
        _mark(SIGN_NONCE_HARNESS, deps)
    return SIGN_NONCE_HARNESS


SIGN_MESSAGE_HARNESS = os.path.join(CSRC, "libdev_sign_message_host.so")


def build_sign_message_harness(force: bool = False) -> str:
    """TEST-ONLY: sign_message_dev.h (the row of sign_message_lane_kernel: encode, hash, sign, store) on the CPU."""
    deps = ["host_sign_message_harness.hip", "host_gtab.h", "sign_message_dev.h", "sign_dev.h", "sha256_dev.h", "recover_dev.h", "modinv_dev.h",
            "secp256k1_dev.h", "keccak_dev.h"]
    if force or _stale(SIGN_MESSAGE_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", SIGN_MESSAGE_HARNESS, os.path.join(CSRC, "host_sign_message_harness.hip")], cwd=CSRC)
        _mark(SIGN_MESSAGE_HARNESS, deps)
    return SIGN_MESSAGE_HARNESS


SIGN_ENVELOPE_HARNESS = os.path.join(CSRC, "libdev_sign_envelope_host.so")


def build_sign_envelope_harness(force: bool = False) -> str:
    """TEST-ONLY: sign_envelope_dev.h (head, body copy, both digest forms, signature: the steps of ibft_sign_envelopes_wire) on the CPU."""
    deps = ["host_sign_envelope_harness.hip", "host_gtab.h", "sign_envelope_dev.h", "sign_message_dev.h", "sign_dev.h", "cert_wave_dev.h", "wave_emul.h",
            "wire_dev.h", "sha256_dev.h", "recover_dev.h", "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h"]
    if force or _stale(SIGN_ENVELOPE_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", SIGN_ENVELOPE_HARNESS, os.path.join(CSRC, "host_sign_envelope_harness.hip")], cwd=CSRC)
        _mark(SIGN_ENVELOPE_HARNESS, deps)
    return SIGN_ENVELOPE_HARNESS


CERT_VERDICT_HARNESS = os.path.join(CSRC, "libdev_cert_verdict_host.so")


def build_cert_verdict_harness(force: bool = False) -> str:
    """TEST-ONLY: cert_verdict_dev.h (validPC and the RoundChangeCertificate rules per carrier: heads, per-child steps, folds) on the CPU."""
    deps = ["host_cert_verdict_harness.hip", "cert_verdict_dev.h", "wire_dev.h", "keccak_dev.h"]
    if force or _stale(CERT_VERDICT_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", CERT_VERDICT_HARNESS, os.path.join(CSRC, "host_cert_verdict_harness.hip")], cwd=CSRC)
        _mark(CERT_VERDICT_HARNESS, deps)
    return CERT_VERDICT_HARNESS


CERT_DECIDE_HARNESS = os.path.join(CSRC, "libdev_cert_decide_host.so")


def build_cert_decide_harness(force: bool = False) -> str:
    """TEST-ONLY: cert_decide_dev.h (the proposer table, valid_pc / round_change per record, the proposal clauses, the selection of
    the highest prepared round) and the resumed sponge of cert_wave_dev.h on the CPU; the cross-lane parts through wave_emul.h."""
    deps = ["host_cert_decide_harness.hip", "cert_decide_dev.h", "cert_verdict_dev.h", "cert_wave_dev.h", "wave_emul.h", "wire_dev.h", "keccak_dev.h"]
    if force or _stale(CERT_DECIDE_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", CERT_DECIDE_HARNESS, os.path.join(CSRC, "host_cert_decide_harness.hip")], cwd=CSRC)
        _mark(CERT_DECIDE_HARNESS, deps)
    return CERT_DECIDE_HARNESS


CERT_DEDUP_HARNESS = os.path.join(CSRC, "libdev_cert_dedup_host.so")


def build_cert_dedup_harness(force: bool = False) -> str:
    """TEST-ONLY: cert_dedup_dev.h (the certificate dedup's table insert, representatives, gather and scatter) on the CPU."""
    deps = ["host_cert_dedup_harness.hip", "cert_dedup_dev.h"]
    if force or _stale(CERT_DEDUP_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", CERT_DEDUP_HARNESS, os.path.join(CSRC, "host_cert_dedup_harness.hip")], cwd=CSRC)
        _mark(CERT_DEDUP_HARNESS, deps)
    return CERT_DEDUP_HARNESS


WIRE_RECODE_HARNESS = os.path.join(CSRC, "libdev_wire_recode_host.so")


def build_wire_recode_harness(force: bool = False) -> str:
    """TEST-ONLY: wire_recode_dev.h (the tolerant walk of IBFT_FLAG_WIRE_RECODE behind the canonical one) on the CPU."""
    deps = ["host_wire_recode_harness.hip", "wire_recode_dev.h", "wire_dev.h", "keccak_dev.h"]
    if force or _stale(WIRE_RECODE_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", WIRE_RECODE_HARNESS, os.path.join(CSRC, "host_wire_recode_harness.hip")], cwd=CSRC)
        _mark(WIRE_RECODE_HARNESS, deps)
    return WIRE_RECODE_HARNESS


WIRE_SETS_HARNESS = os.path.join(CSRC, "libdev_wire_sets_host.so")


def build_wire_sets_harness(force: bool = False) -> str:
    """TEST-ONLY: wire_sets_dev.h (the height map, the row rule and the per-set tally of ibft_verify_senders_wire_sets) and
    tally_dev.h (tally_record) on the CPU."""
    deps = ["host_wire_sets_harness.hip", "wire_sets_dev.h", "tally_dev.h", "wire_dev.h", "recover_dev.h", "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h"]
    if force or _stale(WIRE_SETS_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", WIRE_SETS_HARNESS, os.path.join(CSRC, "host_wire_sets_harness.hip")], cwd=CSRC)
        _mark(WIRE_SETS_HARNESS, deps)
    return WIRE_SETS_HARNESS


WIRE_VIEWS_HARNESS = os.path.join(CSRC, "libdev_wire_views_host.so")


def build_wire_views_harness(force: bool = False) -> str:
    """TEST-ONLY: wire_views_dev.h (the two tables, the stored rule, the ranks and the per-view records of
    ibft_verify_senders_wire_views) on the CPU."""
    deps = ["host_wire_views_harness.hip", "wire_views_dev.h", "wire_sets_dev.h", "tally_dev.h", "wire_dev.h", "cert_decide_dev.h", "cert_verdict_dev.h",
            "recover_dev.h", "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h"]
    if force or _stale(WIRE_VIEWS_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", WIRE_VIEWS_HARNESS, os.path.join(CSRC, "host_wire_views_harness.hip")], cwd=CSRC)
        _mark(WIRE_VIEWS_HARNESS, deps)
    return WIRE_VIEWS_HARNESS


WIRE_VIEW_SEALS_HARNESS = os.path.join(CSRC, "libdev_wire_view_seals_host.so")


def build_wire_view_seals_harness(force: bool = False) -> str:
    """TEST-ONLY: wire_seals_dev.h and the seal form of wire_views_dev.h (the sealable decision, the dense seal rows, the seal
    bits and the COMMIT records of ibft_verify_messages_wire_views) on the CPU."""
    deps = ["host_wire_view_seals_harness.hip", "wire_seals_dev.h", "wire_views_dev.h", "wire_sets_dev.h", "tally_dev.h", "wire_dev.h", "cert_decide_dev.h",
            "cert_verdict_dev.h", "recover_dev.h", "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h"]
    if force or _stale(WIRE_VIEW_SEALS_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", WIRE_VIEW_SEALS_HARNESS, os.path.join(CSRC, "host_wire_view_seals_harness.hip")], cwd=CSRC)
        _mark(WIRE_VIEW_SEALS_HARNESS, deps)
    return WIRE_VIEW_SEALS_HARNESS


ROUND_CHANGE_HARNESS = os.path.join(CSRC, "libdev_round_change_host.so")


def build_round_change_harness(force: bool = False) -> str:
    """TEST-ONLY: round_change_dev.h over wire_views_dev.h's tables (the participation rule, the stored rule, the per-round
    records and the answer of ibft_decide_round_changes_wire) on the CPU; the answer's selection also through wave_emul.h."""
    deps = ["host_round_change_harness.hip", "round_change_dev.h", "wire_views_dev.h", "wire_sets_dev.h", "tally_dev.h", "wire_dev.h", "cert_decide_dev.h",
            "cert_verdict_dev.h", "wave_emul.h", "recover_dev.h", "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h"]
    if force or _stale(ROUND_CHANGE_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", ROUND_CHANGE_HARNESS, os.path.join(CSRC, "host_round_change_harness.hip")], cwd=CSRC)
        _mark(ROUND_CHANGE_HARNESS, deps)
    return ROUND_CHANGE_HARNESS


QTAB_GLV_HARNESS = os.path.join(CSRC, "libdev_qtab_glv_host.so")


def build_qtab_glv_harness(force: bool = False) -> str:
    """TEST-ONLY: the GLV table form of the warm path (verify_dev.h, wave_fe_dev.h) on the CPU; the wavefront form through wave_emul.h."""
    deps = ["host_qtab_glv_harness.hip", "wave_fe_dev.h", "wave_emul.h", "recover_dev.h", "verify_dev.h",
            "modinv_dev.h", "secp256k1_dev.h", "keccak_dev.h", "keccak_row_dev.h"]
    if force or _stale(QTAB_GLV_HARNESS, deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-o", QTAB_GLV_HARNESS, os.path.join(CSRC, "host_qtab_glv_harness.hip")], cwd=CSRC)
        _mark(QTAB_GLV_HARNESS, deps)
    return QTAB_GLV_HARNESS


if __name__ == "__main__":
    print(build_lib(verbose=True))
