"""ctypes binding of libzinc_zip.so (include/zinc_zip_host.h): the C++ mirror of the host side of
zinc::zip -- KeccakTranscript, RaaCode::new, MultilinearZip::{setup, commit, open}, PcsTranscript --
driving the HIP library.  Names and argument meaning follow the reference (src/zip/pcs/*.rs)."""
import ctypes as C
import os

import numpy as np

from . import cabi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libzinc_zip.so")
OK, ERR_INVALID_PARAM, ERR_PANIC, ERR_DEVICE, ERR_NULL, ERR_INVALID_OPEN, ERR_SPARTAN = 0, -1, -2, -3, -4, -5, -6
ERR_FIELD_CONFIG = -7

EXPORTED_SYMBOLS = (
    "zinc_raa_code_new_spec", "zinc_zip_open_challenges", "zinc_commit_z_mle_and_prove_evaluation_spec",
    "zinc_prover_prove_spec", "zinc_verifier_verify_spec", "zinc_verifier_verify_checked_spec",
    "zinc_last_error", "zinc_transcript_new", "zinc_transcript_free", "zinc_transcript_absorb",
    "zinc_transcript_get_u64", "zinc_transcript_get_integer_challenges", "zinc_transcript_get_challenge",
    "zinc_transcript_export", "zinc_transcript_import",
    "zinc_field_constants", "zinc_field_mul", "zinc_map_to_field_i64", "zinc_build_eq_x_r",
    "zinc_shuffle_seeded_perm", "zinc_kat_seed_from_u64", "zinc_raa_code_new", "zinc_zip_setup", "zinc_zip_params_free",
    "zinc_zip_params_geometry", "zinc_zip_commit", "zinc_zip_data_free", "zinc_pcs_transcript_new",
    "zinc_pcs_transcript_free", "zinc_pcs_transcript_len", "zinc_pcs_transcript_copy",
    "zinc_pcs_transcript_probe", "zinc_zip_open", "zinc_pcs_transcript_from_proof", "zinc_pcs_transcript_position",
    "zinc_zip_verify", "zinc_zip_evaluate", "zinc_commit_z_mle_and_prove_evaluation", "zinc_zip_proof_len",
    "zinc_zip_proof_num_roots", "zinc_zip_proof_read", "zinc_zip_proof_free", "zinc_zip_release_cached_contexts", "zinc_sumcheck_prove_product", "zinc_sumcheck_prove_ccs", "zinc_zip_data_download", "zinc_zip_data_upload", "zinc_merkle_tree_new",
    "zinc_prover_prove", "zinc_prover_prepare", "zinc_prepared_ccs_free", "zinc_verifier_verify",
    "zinc_sumcheck_prove_products", "zinc_sumcheck_verify", "zinc_sumcheck_prove_batch", "zinc_prover_prove_batch", "zinc_verifier_verify_batch",
    "zinc_prover_pcs_step_batch",
    "zinc_zip_batch_commit", "zinc_zip_batch_open", "zinc_zip_batch_open_challenges",
    "zinc_zip_batch_verify", "zinc_zip_batch_verify_challenges",
    "zinc_get_prime", "zinc_draw_random_field", "zinc_verifier_verify_checked",
    "zinc_get_prime_batch", "zinc_draw_random_field_batch", "zinc_verifier_check_field_batch",
    "zinc_verifier_verify_batch_checked",
)


class InvalidPcsParam(ValueError):
    """zip::Error::InvalidPcsParam"""


class InvalidPcsOpen(ValueError):
    """zip::Error::InvalidPcsOpen / a transcript read error: the proof is rejected."""


class SpartanError(ValueError):
    """SpartanError / SumCheckError of the verifier (src/zinc/errors.rs)"""


class FieldConfigError(ValueError):
    """ZincError::FieldConfigError: the field the verifier draws from the public input and the transcript
    (draw_random_field, src/zinc/verifier.rs:53-57) is not the configuration it was handed."""


class ReferencePanic(AssertionError):
    """A place where the reference panics (assert! / expect)."""


class DeviceError(RuntimeError):
    pass


class LinearCodeSpec(C.Structure):
    """LinearCodeSpec (src/zip/code.rs:217-242); the defaults are DefaultLinearCodeSpec.  num_proximity_testing = T in
    1 .. 8 reaches the device: T proximity rows in the proof, every one checked by the verifier."""
    _fields_ = [("num_column_opening", C.c_uint32), ("repetition_factor", C.c_uint32), ("num_proximity_testing", C.c_uint32)]

    def __init__(self, num_column_opening=1000, repetition_factor=2, num_proximity_testing=1):
        super().__init__(num_column_opening, repetition_factor, num_proximity_testing)


def _spec_ptr(spec):
    return C.byref(spec) if spec is not None else None


class RaaCodeStruct(C.Structure):
    _fields_ = [("row_len", C.c_uint32), ("repetition_factor", C.c_uint32), ("num_column_opening", C.c_uint32),
                ("num_proximity_testing", C.c_uint32), ("perm_1_seed", C.c_uint64), ("perm_2_seed", C.c_uint64)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        cabi.lib()  # loads torch's HIP runtime first, then libzip_hip.so
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -m zinc_amd.build`")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.zinc_last_error.restype = C.c_char_p
        L.zinc_transcript_new.restype = vp
        L.zinc_transcript_free.argtypes = [vp]
        L.zinc_transcript_absorb.argtypes = [vp, C.c_char_p, C.c_size_t]
        L.zinc_transcript_get_u64.argtypes = [vp]
        L.zinc_transcript_get_u64.restype = C.c_uint64
        L.zinc_transcript_get_integer_challenges.argtypes = [vp, C.c_size_t, vp]
        L.zinc_transcript_get_challenge.argtypes = [vp, vp, C.c_uint32, vp]
        L.zinc_transcript_export.argtypes = [vp, vp, vp, vp]
        L.zinc_transcript_import.argtypes = [vp, vp, vp, C.c_uint32]
        L.zinc_get_prime.argtypes = [vp, C.c_uint32, C.c_int32, vp, C.POINTER(C.c_uint32)]
        L.zinc_draw_random_field.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_int32, vp]
        L.zinc_get_prime_batch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int32, vp, vp]
        L.zinc_draw_random_field_batch.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_int32, vp]
        L.zinc_verifier_check_field_batch.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, C.c_int32, vp]
        L.zinc_field_constants.argtypes = [vp, C.c_uint32, vp, vp, vp]
        L.zinc_field_mul.argtypes = [vp, C.c_uint32, vp, vp, vp]
        L.zinc_map_to_field_i64.argtypes = [vp, C.c_uint32, vp, C.c_size_t, vp]
        L.zinc_build_eq_x_r.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp]
        L.zinc_shuffle_seeded_perm.argtypes = [C.c_uint64, C.c_uint32, vp]
        L.zinc_shuffle_seeded_perm.restype = None
        L.zinc_kat_seed_from_u64.argtypes = [C.c_uint64, vp, C.c_uint32]
        L.zinc_kat_seed_from_u64.restype = None
        L.zinc_raa_code_new.argtypes = [C.c_uint64, vp, C.POINTER(RaaCodeStruct)]
        L.zinc_zip_setup.argtypes = [C.c_uint64, C.POINTER(RaaCodeStruct), C.c_int32, C.POINTER(vp)]
        L.zinc_zip_params_free.argtypes = [vp]
        L.zinc_zip_params_geometry.argtypes = [vp] + [C.POINTER(C.c_uint32)] * 4
        L.zinc_zip_commit.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_int32, vp, C.POINTER(vp)]
        L.zinc_zip_data_free.argtypes = [vp]
        L.zinc_pcs_transcript_new.restype = vp
        L.zinc_pcs_transcript_free.argtypes = [vp]
        L.zinc_pcs_transcript_len.argtypes = [vp]
        L.zinc_pcs_transcript_len.restype = C.c_size_t
        L.zinc_pcs_transcript_copy.argtypes = [vp, vp]
        L.zinc_pcs_transcript_probe.argtypes = [vp]
        L.zinc_pcs_transcript_probe.restype = C.c_uint64
        L.zinc_zip_open.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, vp, C.c_size_t, vp, C.c_uint32, vp]
        L.zinc_zip_batch_commit.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, vp]
        L.zinc_zip_batch_open.argtypes = [vp, vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_uint32, vp]
        L.zinc_zip_batch_open_challenges.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp,
                                                     C.c_size_t, vp, vp]
        L.zinc_zip_batch_verify.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_uint32, vp]
        L.zinc_zip_batch_verify_challenges.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp,
                                                       C.c_size_t, C.c_size_t, vp, vp]
        L.zinc_pcs_transcript_from_proof.argtypes = [vp, C.c_size_t]
        L.zinc_pcs_transcript_from_proof.restype = vp
        L.zinc_pcs_transcript_position.argtypes = [vp]
        L.zinc_pcs_transcript_position.restype = C.c_size_t
        L.zinc_zip_verify.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, C.c_uint32, vp]
        L.zinc_zip_evaluate.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_uint32, vp]
        L.zinc_commit_z_mle_and_prove_evaluation.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp, vp, C.c_uint32,
                                                             C.c_int32, C.POINTER(vp)]
        L.zinc_zip_proof_len.argtypes = [vp]
        L.zinc_zip_proof_len.restype = C.c_size_t
        L.zinc_zip_proof_num_roots.argtypes = [vp]
        L.zinc_zip_proof_num_roots.restype = C.c_size_t
        L.zinc_zip_proof_read.argtypes = [vp, vp, vp, vp]
        L.zinc_zip_proof_read.restype = None
        L.zinc_zip_proof_free.argtypes = [vp]
        L.zinc_sumcheck_prove_ccs.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp,
                                              C.c_uint32, C.c_int32, vp, vp]
        L.zinc_zip_data_download.argtypes = [vp, vp, vp, vp]
        L.zinc_zip_data_upload.argtypes = [vp, vp, vp, vp, C.POINTER(vp)]
        L.zinc_merkle_tree_new.argtypes = [C.c_uint32, vp, C.c_size_t, C.c_uint32, C.c_int32, vp]
        L.zinc_sumcheck_prove_batch.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.c_int32,
                                                vp, vp]
        L.zinc_sumcheck_prove_product.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_int32, vp, vp]
        L.zinc_prover_prove.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_size_t, vp,
                                        C.c_size_t, vp, vp, C.c_uint32, C.c_int32, vp, C.c_int32, vp, vp, vp, vp,
                                        C.POINTER(vp)]
        L.zinc_prover_prove_batch.argtypes = [C.POINTER(LinearCodeSpec), vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp,
                                              C.c_uint32, vp, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
        L.zinc_verifier_verify_batch.argtypes = [C.POINTER(LinearCodeSpec), vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp,
                                                 C.c_uint32, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t]
        L.zinc_verifier_verify_batch_checked.argtypes = [vp, vp] + L.zinc_verifier_verify_batch.argtypes
        L.zinc_prover_pcs_step_batch.argtypes = [C.POINTER(LinearCodeSpec), C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, C.c_int32, vp]
        L.zinc_prover_prepare.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_int32, C.POINTER(vp)]
        L.zinc_prepared_ccs_free.argtypes = [vp]
        L.zinc_prepared_ccs_free.restype = None
        L.zinc_sumcheck_verify.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp]
        L.zinc_sumcheck_prove_products.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp,
                                                   C.c_uint32, C.c_int32, vp, vp]
        L.zinc_verifier_verify.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint32,
                                           C.c_int32, vp, vp, vp, vp, C.c_int32, vp, C.c_size_t, vp, vp, C.c_size_t,
                                           vp, vp, vp]
        L.zinc_verifier_verify_checked.argtypes = [vp, C.c_size_t, C.c_int32] + L.zinc_verifier_verify.argtypes
        # the _spec variants: the LinearCodeSpec first (NULL = the default), then the arguments of the plain function
        sp = C.POINTER(LinearCodeSpec)
        L.zinc_raa_code_new_spec.argtypes = [sp] + L.zinc_raa_code_new.argtypes
        L.zinc_commit_z_mle_and_prove_evaluation_spec.argtypes = [sp] + L.zinc_commit_z_mle_and_prove_evaluation.argtypes
        L.zinc_prover_prove_spec.argtypes = [sp] + L.zinc_prover_prove.argtypes
        L.zinc_verifier_verify_spec.argtypes = [sp] + L.zinc_verifier_verify.argtypes
        L.zinc_verifier_verify_checked_spec.argtypes = [sp] + L.zinc_verifier_verify_checked.argtypes
        L.zinc_zip_open_challenges.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp]
        _lib = L
    return _lib


def _error(rc, msg):
    """the exception object of a facade return code (None for OK)"""
    if rc == OK:
        return None
    if rc == ERR_INVALID_PARAM:
        return InvalidPcsParam(msg)
    if rc == ERR_INVALID_OPEN:
        return InvalidPcsOpen(msg)
    if rc == ERR_PANIC:
        return ReferencePanic(msg)
    if rc == ERR_SPARTAN:
        return SpartanError(msg)
    if rc == ERR_FIELD_CONFIG:
        return FieldConfigError(msg)
    return DeviceError(msg)


def _check(rc):
    if rc == OK:
        return
    raise _error(rc, lib().zinc_last_error().decode())


def _limbs(value: int, n: int) -> np.ndarray:
    return np.array([(value >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)], dtype=np.uint64)


class FieldConfig:
    """FieldConfig::new(modulus) with FIELD_LIMBS = limbs."""

    def __init__(self, modulus: int, limbs: int):
        self.modulus, self.limbs = modulus, limbs
        self._m = _limbs(modulus, limbs)

    def constants(self):
        r, r2 = np.zeros(self.limbs, np.uint64), np.zeros(self.limbs, np.uint64)
        inv = C.c_uint64()
        _check(lib().zinc_field_constants(self._m.ctypes.data, self.limbs, r.ctypes.data, r2.ctypes.data, C.byref(inv)))
        return r, r2, inv.value

    def mul(self, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        out = np.zeros(self.limbs, np.uint64)
        a, b = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b, np.uint64)
        _check(lib().zinc_field_mul(self._m.ctypes.data, self.limbs, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def map_to_field(self, values) -> np.ndarray:
        v = np.ascontiguousarray(values, dtype=np.int64)
        out = np.zeros((v.size, self.limbs), np.uint64)
        _check(lib().zinc_map_to_field_i64(self._m.ctypes.data, self.limbs, v.ctypes.data, v.size, out.ctypes.data))
        return out

    def build_eq_x_r(self, r: np.ndarray) -> np.ndarray:
        r = np.ascontiguousarray(r, np.uint64)
        out = np.zeros((1 << r.shape[0], self.limbs), np.uint64)
        _check(lib().zinc_build_eq_x_r(self._m.ctypes.data, self.limbs, r.ctypes.data, r.shape[0], out.ctypes.data))
        return out


class KeccakTranscript:
    def __init__(self):
        self._h = lib().zinc_transcript_new()

    def __del__(self):
        try:  # (at interpreter shutdown the module globals may already be gone)
            if getattr(self, "_h", None):
                lib().zinc_transcript_free(self._h)
                self._h = None
        except Exception:
            pass

    def absorb(self, data: bytes):
        lib().zinc_transcript_absorb(self._h, data, len(data))

    def get_u64(self) -> int:
        return lib().zinc_transcript_get_u64(self._h)

    def get_integer_challenges(self, n: int) -> np.ndarray:
        out = np.zeros(n, np.int64)
        lib().zinc_transcript_get_integer_challenges(self._h, n, out.ctypes.data)
        return out

    def get_challenge(self, field: FieldConfig) -> np.ndarray:
        out = np.zeros(field.limbs, np.uint64)
        _check(lib().zinc_transcript_get_challenge(self._h, field._m.ctypes.data, field.limbs, out.ctypes.data))
        return out

    def state(self):
        """The Keccak-256 sponge in transit: (st [25] uint64: the state after every full block, buf: the bytes
        absorbed since) -- the fields of zip_keccak_state, what cabi.Sumcheck.prove borrows."""
        st, buf, n = np.zeros(25, np.uint64), np.zeros(136, np.uint8), C.c_uint32(0)
        _check(lib().zinc_transcript_export(self._h, st.ctypes.data, buf.ctypes.data, C.addressof(n)))
        return st, buf[: n.value].tobytes()

    def set_state(self, state):
        st, buf = state
        st = np.ascontiguousarray(st, dtype=np.uint64)
        if st.shape != (25,):
            raise ValueError("the Keccak state has 25 words")
        room = np.zeros(136, np.uint8)
        room[: min(len(buf), 136)] = np.frombuffer(bytes(buf[:136]), np.uint8)
        _check(lib().zinc_transcript_import(self._h, st.ctypes.data, room.ctypes.data, len(buf)))


def get_prime(transcript: KeccakTranscript, limbs: int, device: int = 0, want_tried: bool = False):
    """prime_gen::get_prime::<RandomField<limbs>>(transcript) (src/prime_gen.rs:15-28): the first candidate of the
    transcript's hash chain that MillerRabin::test_base_two accepts, as a Python int; the candidates of a batch are
    tested in one launch on the device.  The transcript ends where the reference's loop leaves it.
    want_tried: -> (prime, the winner's 1-based position in the chain)."""
    out = np.zeros(limbs, np.uint64)
    tried = C.c_uint32(0)
    _check(lib().zinc_get_prime(transcript._h, limbs, device, out.ctypes.data, C.byref(tried)))
    prime = sum(int(w) << (64 * i) for i, w in enumerate(out))
    return (prime, tried.value) if want_tried else prime


def draw_random_field(public_input, transcript: KeccakTranscript, limbs: int, device: int = 0) -> FieldConfig:
    """draw_random_field::<Int<1>, RandomField<limbs>> (src/zinc/utils.rs:161-171): absorbs every public input as its 8
    little-endian bytes, then FieldConfig::new(get_prime(transcript))."""
    x = np.ascontiguousarray(public_input, dtype=np.int64).reshape(-1)
    out = np.zeros(limbs, np.uint64)
    _check(lib().zinc_draw_random_field(x.ctypes.data if x.size else None, x.size, transcript._h, limbs, device,
                                        out.ctypes.data))
    return FieldConfig(sum(int(w) << (64 * i) for i, w in enumerate(out)), limbs)


def _public_inputs(public_inputs):
    """-> (kept arrays, the pointer array, the length array) of one int64 public input per member"""
    xs = [np.ascontiguousarray(x, dtype=np.int64).reshape(-1) for x in public_inputs]
    n = max(len(xs), 1)
    ptrs = (C.c_void_p * n)(*[x.ctypes.data if x.size else None for x in xs])
    lens = (C.c_size_t * n)(*[x.size for x in xs])
    return xs, ptrs, lens


def get_prime_batch(transcripts, limbs: int, device: int = 0, want_tried: bool = False):
    """get_prime for every transcript of a batch (prime_gen::get_prime_batch): from the line profiles/prime_batch.md sets
    on (ZIP_HIP_PRIME_MIN_BATCH=n moves it) ONE zip_get_prime_batch call, the candidate chains and the tests on the device;
    below it, and with ZIP_HIP_BATCH=0, the loop over get_prime -- the same primes and transcripts either way.
    -> the primes as Python ints; want_tried: -> (primes, the winners' 1-based positions)."""
    n = len(transcripts)
    trs = (C.c_void_p * max(n, 1))(*[t._h for t in transcripts])
    out = np.zeros((max(n, 1), limbs), np.uint64)
    tried = np.zeros(max(n, 1), np.uint32)
    _check(lib().zinc_get_prime_batch(trs, n, limbs, device, out.ctypes.data, tried.ctypes.data))
    primes = [sum(int(w) << (64 * i) for i, w in enumerate(out[k])) for k in range(n)]
    return (primes, [int(x) for x in tried[:n]]) if want_tried else primes


def draw_random_field_batch(public_inputs, transcripts, limbs: int, device: int = 0):
    """draw_random_field for every member of a batch: member i absorbs public_inputs[i] on transcripts[i], then one
    get_prime_batch over all of them -> a FieldConfig per member."""
    n = len(transcripts)
    assert len(public_inputs) == n
    _keep, ptrs, lens = _public_inputs(public_inputs)
    trs = (C.c_void_p * max(n, 1))(*[t._h for t in transcripts])
    out = np.zeros((max(n, 1), limbs), np.uint64)
    _check(lib().zinc_draw_random_field_batch(ptrs, lens, trs, n, limbs, device, out.ctypes.data))
    return [FieldConfig(sum(int(w) << (64 * i) for i, w in enumerate(out[k])), limbs) for k in range(n)]


def kat_seed_from_u64(seed: int, n_words: int):
    out = np.zeros(n_words, np.uint32)
    lib().zinc_kat_seed_from_u64(seed, out.ctypes.data, n_words)
    return [int(x) for x in out]


def shuffle_seeded_perm(seed: int, length: int) -> np.ndarray:
    out = np.zeros(length, np.uint32)
    lib().zinc_shuffle_seeded_perm(seed, length, out.ctypes.data)
    return out


class RaaCode:
    """RaaCode::new(spec, poly_size, transcript); spec=None -> DefaultLinearCodeSpec, transcript=None -> MockTranscript."""

    def __init__(self, poly_size: int, transcript: KeccakTranscript = None, spec: "LinearCodeSpec" = None):
        self.s = RaaCodeStruct()
        _check(lib().zinc_raa_code_new_spec(_spec_ptr(spec), poly_size, transcript._h if transcript else None, C.byref(self.s)))
        self.poly_size = poly_size

    row_len = property(lambda self: self.s.row_len)
    perm_1_seed = property(lambda self: self.s.perm_1_seed)
    perm_2_seed = property(lambda self: self.s.perm_2_seed)

    def codeword_len(self):
        return self.s.row_len * self.s.repetition_factor


class PcsTranscript:
    def __init__(self, _handle=None):
        self._h = _handle if _handle is not None else lib().zinc_pcs_transcript_new()

    @classmethod
    def from_proof(cls, proof) -> "PcsTranscript":
        p = np.ascontiguousarray(proof, dtype=np.uint8)
        return cls(lib().zinc_pcs_transcript_from_proof(p.ctypes.data, p.size))

    def position(self) -> int:
        return lib().zinc_pcs_transcript_position(self._h)

    def __del__(self):
        try:  # (at interpreter shutdown the module globals may already be gone)
            if getattr(self, "_h", None):
                lib().zinc_pcs_transcript_free(self._h)
                self._h = None
        except Exception:
            pass

    def into_proof(self) -> np.ndarray:
        out = np.zeros(lib().zinc_pcs_transcript_len(self._h), np.uint8)
        if out.size:
            lib().zinc_pcs_transcript_copy(self._h, out.ctypes.data)
        return out

    def probe(self) -> int:
        return lib().zinc_pcs_transcript_probe(self._h)


class MerkleTree:
    """MerkleTree {root, depth, layers} (src/zip/pcs/utils.rs:67-85)."""

    def __init__(self, depth: int, layers: np.ndarray, root: np.ndarray):
        self.depth, self.layers, self.root = depth, layers, root

    @classmethod
    def new(cls, depth: int, leaves, device: int = 0) -> "MerkleTree":
        lv = np.ascontiguousarray(leaves, dtype=np.uint64)
        lv = lv.reshape(lv.shape[0], -1)
        out = np.zeros(((2 << depth) - 1, 32), np.uint8)
        _check(lib().zinc_merkle_tree_new(depth, lv.ctypes.data, lv.shape[0], lv.shape[1], device, out.ctypes.data))
        return cls(depth, out[:-1], out[-1])


class MultilinearZipData:
    """MultilinearZipData {rows, rows_merkle_trees} (structs.rs:33-38), resident on the device; `rows` and
    `rows_merkle_trees` copy it to the host, `new` builds a handle from (possibly modified) host data."""

    def __init__(self, handle, pp=None, has_trees=True):
        self._h, self._pp, self._has_trees = handle, pp, has_trees

    @property
    def rows(self) -> np.ndarray:
        pp = self._pp
        out = np.zeros((pp.num_rows * pp.codeword_len, 4), np.uint64)
        _check(lib().zinc_zip_data_download(self._h, out.ctypes.data, None, None))
        return out

    @property
    def rows_merkle_trees(self):
        pp = self._pp
        if not self._has_trees:
            return []
        depth = pp.codeword_len.bit_length() - 1
        layers = np.zeros((pp.num_rows, 2 * pp.codeword_len - 2, 32), np.uint8)
        roots = np.zeros((pp.num_rows, 32), np.uint8)
        _check(lib().zinc_zip_data_download(self._h, None, layers.ctypes.data, roots.ctypes.data))
        return [MerkleTree(depth, layers[r], roots[r]) for r in range(pp.num_rows)]

    @classmethod
    def new(cls, pp, rows, rows_merkle_trees) -> "MultilinearZipData":
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        layers = np.ascontiguousarray(np.stack([t.layers for t in rows_merkle_trees]), dtype=np.uint8)
        roots = np.ascontiguousarray(np.stack([t.root for t in rows_merkle_trees]), dtype=np.uint8)
        h = C.c_void_p()
        _check(lib().zinc_zip_data_upload(pp._h, r.ctypes.data, layers.ctypes.data, roots.ctypes.data, C.byref(h)))
        return cls(h, pp, True)

    def __del__(self):
        try:  # (at interpreter shutdown the module globals may already be gone)
            if getattr(self, "_h", None):
                lib().zinc_zip_data_free(self._h)
                self._h = None
        except Exception:
            pass


class MultilinearZipParams:
    def __init__(self, handle):
        self._h = handle
        g = [C.c_uint32() for _ in range(4)]
        lib().zinc_zip_params_geometry(handle, *[C.byref(x) for x in g])
        self.num_vars, self.num_rows, self.row_len, self.codeword_len = [x.value for x in g]

    def __del__(self):
        try:  # (at interpreter shutdown the module globals may already be gone)
            if getattr(self, "_h", None):
                lib().zinc_zip_params_free(self._h)
                self._h = None
        except Exception:
            pass


class MultilinearZip:
    @staticmethod
    def setup(poly_size: int, linear_code: RaaCode, device: int = 0) -> MultilinearZipParams:
        h = C.c_void_p()
        _check(lib().zinc_zip_setup(poly_size, C.byref(linear_code.s), device, C.byref(h)))
        return MultilinearZipParams(h)

    @staticmethod
    def commit(pp: MultilinearZipParams, evaluations, num_vars: int = None, with_merkle: bool = True):
        ev = np.ascontiguousarray(evaluations, dtype=np.int64)
        nv = num_vars if num_vars is not None else max(ev.size, 1).bit_length() - 1
        roots = np.zeros((pp.num_rows, 32), np.uint8)
        h = C.c_void_p()
        _check(lib().zinc_zip_commit(pp._h, ev.ctypes.data, ev.size, nv, int(with_merkle), roots.ctypes.data, C.byref(h)))
        return MultilinearZipData(h, pp, with_merkle), (roots if with_merkle else None)

    @staticmethod
    def commit_no_merkle(pp: MultilinearZipParams, evaluations, num_vars: int = None):
        """commit.rs:104-119: (data with empty trees, commitment with no roots)"""
        data, _ = MultilinearZip.commit(pp, evaluations, num_vars, with_merkle=False)
        return data, np.zeros((0, 32), np.uint8)

    @staticmethod
    def encode_rows(pp: MultilinearZipParams, evaluations) -> np.ndarray:
        """commit.rs:158-183: the encoded rows as a flat vector of Int<4>"""
        return MultilinearZip.commit_no_merkle(pp, evaluations)[0].rows

    @staticmethod
    def batch_commit(pp: MultilinearZipParams, polys):
        """commit.rs:134-142: one device batch, one commit launch for all polynomials (zinc_zip_batch_commit)
        -> [(MultilinearZipData, roots)]"""
        evs = [np.ascontiguousarray(p, dtype=np.int64) for p in polys]
        m = len(evs)
        if not m:
            return []
        ptrs = (C.c_void_p * m)(*[e.ctypes.data for e in evs])
        sizes = (C.c_size_t * m)(*[e.size for e in evs])
        nvs = (C.c_uint32 * m)(*[max(e.size, 1).bit_length() - 1 for e in evs])
        roots = np.zeros((m, pp.num_rows, 32), np.uint8)
        outs = (C.c_void_p * m)()
        rc = lib().zinc_zip_batch_commit(pp._h, ptrs, sizes, nvs, m, roots.ctypes.data, outs)
        datas = [MultilinearZipData(C.c_void_p(h), pp, True) for h in outs if h]  # (adopted first: freed if the call failed)
        _check(rc)
        return [(d, roots[i]) for i, d in enumerate(datas)]

    @staticmethod
    def batch_open(pp: MultilinearZipParams, polys, datas, points, field: "FieldConfig", transcript: "PcsTranscript"):
        """open_z.rs:43-58 (zinc_zip_batch_open): batched on the device when `datas` are all the members of one
        batch_commit, in order; the loop over open otherwise"""
        evs = [np.ascontiguousarray(p, dtype=np.int64) for p in polys]
        m = min(len(evs), len(datas), len(points))
        if not m:
            return
        pts = [np.ascontiguousarray(pt, dtype=np.uint64).reshape(-1, field.limbs) if np.size(pt) else np.zeros((0, field.limbs), np.uint64)
               for pt in points[:m]]
        nv = [max(e.size, 1).bit_length() - 1 for e in evs[:m]]
        for i in range(m):
            if pts[i].shape[0] != nv[i]:  # validate_input (pcs/utils.rs:24-58): the loop raises the reference's error
                for p, d, pt in zip(polys, datas, points):
                    MultilinearZip.open(pp, p, d, pt, field, transcript)
                return
        ptrs = (C.c_void_p * m)(*[e.ctypes.data for e in evs[:m]])
        sizes = (C.c_size_t * m)(*[e.size for e in evs[:m]])
        nvs = (C.c_uint32 * m)(*nv)
        dh = (C.c_void_p * m)(*[d._h if isinstance(d._h, int) else d._h.value for d in datas[:m]])
        pp_ = (C.c_void_p * m)(*[pt.ctypes.data for pt in pts])
        _check(lib().zinc_zip_batch_open(pp._h, ptrs, sizes, nvs, dh, pp_, m, field._m.ctypes.data, field.limbs, transcript._h))

    @staticmethod
    def batch_verify_z(vp: MultilinearZipParams, comms, points, evals, transcript: "PcsTranscript", field: "FieldConfig"):
        """verify_z.rs:40-58 (zinc_zip_batch_verify): one host walk of the shared transcript and one device call for all
        polynomials where the batch serves them, the loop over verify otherwise.  Returns None when every proof is accepted;
        raises what verify raises for the first rejected polynomial and leaves the transcript where the loop leaves it."""
        m = min(len(comms), len(points), len(evals))
        if not m:
            return
        roots = np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.uint8).reshape(-1) for c in comms[:m]]))
        pts = [np.ascontiguousarray(pt, dtype=np.uint64).reshape(-1, field.limbs) if np.size(pt) else np.zeros((0, field.limbs), np.uint64)
               for pt in points[:m]]
        ptrs = (C.c_void_p * m)(*[pt.ctypes.data for pt in pts])
        lens = (C.c_size_t * m)(*[pt.shape[0] for pt in pts])
        ev = np.ascontiguousarray(np.stack([np.asarray(e, dtype=np.uint64).reshape(-1)[:field.limbs] for e in evals[:m]]))
        _check(lib().zinc_zip_batch_verify(vp._h, roots.ctypes.data, ptrs, lens, ev.ctypes.data, m, field._m.ctypes.data,
                                           field.limbs, transcript._h))

    @staticmethod
    def open_challenges(num_rows: int, codeword_len: int, num_column_opening: int, num_proximity_testing: int,
                        field: "FieldConfig", transcript: "PcsTranscript"):
        """The squeezes of prove_testing_phase / verify_testing and nothing else (host only): per proximity test
        get_integer_challenges(num_rows) if num_rows > 1, then the column indices -> (coeffs [T, num_rows] or None, cols).
        InvalidPcsParam for num_proximity_testing outside 1 .. 8 when num_rows > 1."""
        n_coeffs = num_proximity_testing * num_rows if num_rows > 1 and 1 <= num_proximity_testing <= 8 else 0
        coeffs = np.zeros(max(n_coeffs, 1), np.int64)
        cols = np.zeros(max(num_column_opening, 1), np.uint32)
        _check(lib().zinc_zip_open_challenges(num_rows, codeword_len, num_column_opening, num_proximity_testing,
                                              field._m.ctypes.data, field.limbs, transcript._h, coeffs.ctypes.data,
                                              cols.ctypes.data))
        return (coeffs[:n_coeffs].reshape(num_proximity_testing, num_rows) if n_coeffs else None), cols[:num_column_opening]

    @staticmethod
    def open(pp: MultilinearZipParams, evaluations, commit_data: MultilinearZipData, point: np.ndarray,
             field: FieldConfig, transcript: PcsTranscript, num_vars: int = None):
        ev = np.ascontiguousarray(evaluations, dtype=np.int64)
        nv = num_vars if num_vars is not None else max(ev.size, 1).bit_length() - 1
        pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, field.limbs) if np.size(point) else np.zeros((0, field.limbs), np.uint64)
        _check(lib().zinc_zip_open(pp._h, ev.ctypes.data, ev.size, nv, commit_data._h, pt.ctypes.data, pt.shape[0],
                                   field._m.ctypes.data, field.limbs, transcript._h))

    @staticmethod
    def verify(vp: MultilinearZipParams, roots, point: np.ndarray, eval_mont, field: FieldConfig,
               transcript: PcsTranscript):
        """MultilinearZip::verify: returns None when the proof is accepted, raises InvalidPcsOpen otherwise."""
        r = np.ascontiguousarray(roots, dtype=np.uint8)
        pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, field.limbs) if np.size(point) else np.zeros((0, field.limbs), np.uint64)
        ev = np.ascontiguousarray(eval_mont, dtype=np.uint64)
        _check(lib().zinc_zip_verify(vp._h, r.ctypes.data, pt.ctypes.data, pt.shape[0], ev.ctypes.data,
                                     field._m.ctypes.data, field.limbs, transcript._h))

    @staticmethod
    def evaluate(pp: MultilinearZipParams, evaluations, point: np.ndarray, field: FieldConfig) -> np.ndarray:
        """z_mle.map_to_field(config).evaluate(point) (zinc/prover.rs:317-319)."""
        ev = np.ascontiguousarray(evaluations, dtype=np.int64)
        pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, field.limbs) if np.size(point) else np.zeros((0, field.limbs), np.uint64)
        out = np.zeros(field.limbs, np.uint64)
        _check(lib().zinc_zip_evaluate(pp._h, ev.ctypes.data, ev.size, pt.ctypes.data, pt.shape[0], field._m.ctypes.data,
                                       field.limbs, out.ctypes.data))
        return out


def commit_z_mle_and_prove_evaluation(z_evals, r_y: np.ndarray, transcript: KeccakTranscript, field: FieldConfig,
                                      device: int = 0, spec: "LinearCodeSpec" = None):
    """ZincProver::commit_z_mle_and_prove_evaluation (src/zinc/prover.rs:305-327) -> (roots, v, pcs_proof)."""
    ev = np.ascontiguousarray(z_evals, dtype=np.int64)
    pt = np.ascontiguousarray(r_y, dtype=np.uint64).reshape(-1, field.limbs) if np.size(r_y) else np.zeros((0, field.limbs), np.uint64)
    h = C.c_void_p()
    _check(lib().zinc_commit_z_mle_and_prove_evaluation_spec(_spec_ptr(spec), ev.ctypes.data, ev.size, pt.ctypes.data,
                                                             pt.shape[0], transcript._h, field._m.ctypes.data, field.limbs,
                                                             device, C.byref(h)))
    try:
        roots = np.zeros((lib().zinc_zip_proof_num_roots(h), 32), np.uint8)
        v = np.zeros(field.limbs, np.uint64)
        proof = np.zeros(lib().zinc_zip_proof_len(h), np.uint8)
        lib().zinc_zip_proof_read(h, roots.ctypes.data, v.ctypes.data, proof.ctypes.data)
    finally:
        lib().zinc_zip_proof_free(h)
    return roots, v, proof


def sumcheck_prove_product(transcript: KeccakTranscript, mles, degree: int, field: FieldConfig, device: int = 0):
    """MLSumcheck::prove_as_subprotocol for comb_fn = product of the MLEs (src/sumcheck.rs:56-112).
    mles: [K, 2^nv, limbs] Montgomery limbs.  Returns (msgs [nv, degree+1, limbs], randomness [nv, limbs])."""
    m = np.ascontiguousarray(mles, dtype=np.uint64)
    K, n, fl = m.shape
    nv = n.bit_length() - 1
    ptrs = (C.c_void_p * K)(*[m[k].ctypes.data for k in range(K)])
    msgs = np.zeros((nv, degree + 1, fl), np.uint64)
    rand = np.zeros((nv, fl), np.uint64)
    _check(lib().zinc_sumcheck_prove_product(transcript._h, ptrs, K, nv, degree, field._m.ctypes.data, fl, device,
                                             msgs.ctypes.data, rand.ctypes.data))
    return msgs, rand


def sumcheck_prove_ccs(transcript: KeccakTranscript, mles, degree: int, c, S, field: FieldConfig, device: int = 0):
    """prove_as_subprotocol with sumcheck_polynomial_comb_fn_1 (zinc/utils.rs:77-94): c = ccs.c as [n_terms, limbs]
    Montgomery limbs, S = ccs.S (lists of positions in `mles`, the eq() MLE last)."""
    m = np.ascontiguousarray(mles, dtype=np.uint64)
    K, n, fl = m.shape
    nv = n.bit_length() - 1
    ptrs = (C.c_void_p * K)(*[m[k].ctypes.data for k in range(K)])
    cv = np.ascontiguousarray(c, dtype=np.uint64).reshape(len(S), fl)
    masks = np.array([sum(1 << j for j in s) for s in S], dtype=np.uint32)
    msgs = np.zeros((nv, degree + 1, fl), np.uint64)
    rand = np.zeros((nv, fl), np.uint64)
    _check(lib().zinc_sumcheck_prove_ccs(transcript._h, ptrs, K, nv, degree, len(S), cv.ctypes.data, masks.ctypes.data,
                                         field._m.ctypes.data, fl, device, msgs.ctypes.data, rand.ctypes.data))
    return msgs, rand


def sumcheck_prove_batch(transcripts, mles, degree: int, fields, combs=None, device: int = 0):
    """Many small sumchecks of one shape: on instance i what sumcheck_prove_product (combs is None or combs[i] is None)
    or sumcheck_prove_ccs (combs[i] = (c, S) as there) does with transcripts[i], mles[i] ([K, 2^nv, limbs]) and fields[i].
    From 2 / 3 / 6 instances on (up to 12 / 14 / 16 variables) it is one zip_sumcheck_prove_batch call (ZIP_HIP_BATCH=0,
    more than 16 variables or fields of different limb counts: the loop).  Returns the lists ([msgs [nv, degree+1, limbs] ...], [randomness [nv, limbs] ...])."""
    B = len(transcripts)
    tabs = [np.ascontiguousarray(m, dtype=np.uint64) for m in mles]
    K, n, _ = tabs[0].shape
    nv = n.bit_length() - 1
    assert all(t.shape[:2] == (K, n) for t in tabs) and len(tabs) == B and len(fields) == B
    ptrs = (C.c_void_p * (B * K))(*[t[k].ctypes.data for t in tabs for k in range(K)])
    trs = (C.c_void_p * B)(*[t._h for t in transcripts])
    limbs = np.array([f.limbs for f in fields], dtype=np.uint32)
    moduli = np.zeros((B, 4), dtype=np.uint64)
    n_terms = np.zeros(B, dtype=np.uint32)
    cv = np.zeros((B, 8, 4), dtype=np.uint64)
    masks = np.zeros((B, 8), dtype=np.uint32)
    for i, f in enumerate(fields):
        moduli[i, :f.limbs] = np.asarray(f._m, dtype=np.uint64)[:f.limbs]
        if combs is not None and combs[i] is not None:
            c, S = combs[i]
            n_terms[i] = len(S)
            cv[i, :len(S), :f.limbs] = np.asarray(c, dtype=np.uint64).reshape(len(S), f.limbs)
            masks[i, :len(S)] = [sum(1 << j for j in s) for s in S]
    total = int(limbs.sum())
    msgs = np.zeros(nv * (degree + 1) * total, np.uint64)
    rand = np.zeros(nv * total, np.uint64)
    _check(lib().zinc_sumcheck_prove_batch(trs, B, ptrs, K, nv, degree, n_terms.ctypes.data, cv.ctypes.data, masks.ctypes.data,
                                           moduli.ctypes.data, limbs.ctypes.data, device, msgs.ctypes.data, rand.ctypes.data))
    out_m, out_r, m_at, r_at = [], [], 0, 0
    for fl in (int(x) for x in limbs):
        out_m.append(msgs[m_at:m_at + nv * (degree + 1) * fl].reshape(nv, degree + 1, fl))
        out_r.append(rand[r_at:r_at + nv * fl].reshape(nv, fl))
        m_at += nv * (degree + 1) * fl
        r_at += nv * fl
    return out_m, out_r


def sumcheck_prove_products(transcript: KeccakTranscript, mles, degree: int, masks, coeffs, field: FieldConfig,
                            device: int = 0, nvars: int = None):
    """prove_as_subprotocol with rand_poly_comb_fn (sumcheck/utils.rs:67-78): sum_p coeffs[p] * prod_{j in masks[p]} vals[j].
    mles: [K, 2^nv, limbs] Montgomery limbs; coeffs: [P, limbs]; masks: P bit masks over the K MLEs."""
    m = np.ascontiguousarray(mles, dtype=np.uint64)
    K, n, fl = m.shape
    nv = nvars if nvars is not None else n.bit_length() - 1
    ptrs = (C.c_void_p * max(K, 1))(*[m[k].ctypes.data for k in range(K)])
    mk = np.ascontiguousarray(masks, dtype=np.uint32)
    cv = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(mk.size, fl) if mk.size else np.zeros((1, fl), np.uint64)
    msgs = np.zeros((nv, degree + 1, fl), np.uint64)
    rand = np.zeros((nv, fl), np.uint64)
    if not mk.size:
        mk = np.zeros(1, np.uint32)  # (a valid pointer; n_products == 0 says nothing is read)
        n_products = 0
    else:
        n_products = mk.size
    _check(lib().zinc_sumcheck_prove_products(transcript._h, ptrs, K, nv, degree, n_products, cv.ctypes.data, mk.ctypes.data,
                                              field._m.ctypes.data, fl, device, msgs.ctypes.data, rand.ctypes.data))
    return msgs, rand


def sumcheck_verify(transcript: KeccakTranscript, nvars: int, degree: int, claimed_sum, msgs, field: FieldConfig):
    """MLSumcheck::verify_as_subprotocol -> (point [nvars, limbs], expected_evaluation [limbs]); raises SpartanError.
    msgs: [rounds, evaluations per round, limbs] -- whatever the proof holds, also when that is the wrong shape."""
    fl = field.limbs
    m = np.ascontiguousarray(msgs, dtype=np.uint64).reshape(-1, np.shape(msgs)[1] if np.ndim(msgs) == 3 else 0, fl) \
        if np.size(msgs) else np.zeros((0, 0, fl), np.uint64)
    cs = np.ascontiguousarray(claimed_sum, dtype=np.uint64).reshape(fl)
    point = np.zeros((max(nvars, 1), fl), np.uint64)
    expected = np.zeros(fl, np.uint64)
    _check(lib().zinc_sumcheck_verify(transcript._h, nvars, degree, cs.ctypes.data, m.ctypes.data if m.size else None,
                                      m.shape[0], m.shape[1], field._m.ctypes.data, fl, point.ctypes.data, expected.ctypes.data))
    return point[:nvars], expected


class ZincProver:
    """ZincProver (src/zinc/structs.rs:33-47, src/zinc/prover.rs).  A CCS is given as
      matrices  Statement_Z.constraints: objects with n_rows, n_cols, row_ptr, col_idx (uint32), values (int64)  [CSR]
      s, d, S, c  CCS_Z with m = n = 2^s = 2^s_prime
      public_input, w_ccs  Statement_Z.public_input, Witness_Z.w_ccs (z = x || 1 || w)
    spec: the LinearCodeSpec of ZincProver::new (None: the default)."""

    def __init__(self, device: int = 0, spec: "LinearCodeSpec" = None):
        self.device = device
        self.spec = spec

    @staticmethod
    def _abi_matrices(matrices):
        keep = [(np.ascontiguousarray(M.row_ptr, dtype=np.uint32), np.ascontiguousarray(M.col_idx, dtype=np.uint32),
                 np.ascontiguousarray(M.values, dtype=np.int64)) for M in matrices]
        arr = (cabi.SparseMatrix * len(matrices))()
        for k, (M, (rp, ci, va)) in enumerate(zip(matrices, keep)):
            arr[k] = cabi.SparseMatrix(M.n_rows, M.n_cols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data)
        return arr, keep

    def prepare(self, matrices, s, field: "FieldConfig") -> "PreparedCcs":
        """The circuit's matrices in F_q on the device, for every later proof of that circuit (PreparedCcs)."""
        arr, _keep = self._abi_matrices(matrices)
        h = C.c_void_p()
        _check(lib().zinc_prover_prepare(arr, len(matrices), s, field._m.ctypes.data, field.limbs, self.device, C.byref(h)))
        return PreparedCcs(h)

    def _run(self, matrices, s, d, S, c, public_input, w_ccs, transcript, field, with_pcs, prepared=None):
        t, fl = len(matrices), field.limbs
        arr, _keep = self._abi_matrices(matrices)
        masks = np.array([sum(1 << j for j in Si) for Si in S], dtype=np.uint32)
        cv = np.array(c, dtype=np.int64)
        x = np.ascontiguousarray(public_input, dtype=np.int64)
        w = np.ascontiguousarray(w_ccs, dtype=np.int64)
        out = dict(msgs1=np.zeros((s, d + 2, fl), np.uint64), msgs2=np.zeros((s, 3, fl), np.uint64),
                   V_s=np.zeros((t, fl), np.uint64), r_y=np.zeros((s, fl), np.uint64))
        h = C.c_void_p()
        _check(lib().zinc_prover_prove_spec(_spec_ptr(self.spec), arr, t, s, d, len(S), masks.ctypes.data, cv.ctypes.data, x.ctypes.data, x.size,
                                       w.ctypes.data, w.size, transcript._h, field._m.ctypes.data, fl, self.device,
                                       prepared._h if prepared is not None else None, 1 if with_pcs else 0, out["msgs1"].ctypes.data, out["msgs2"].ctypes.data,
                                       out["V_s"].ctypes.data, out["r_y"].ctypes.data, C.byref(h)))
        if with_pcs:
            try:
                roots = np.zeros((lib().zinc_zip_proof_num_roots(h), 32), np.uint8)
                v = np.zeros(fl, np.uint64)
                proof = np.zeros(lib().zinc_zip_proof_len(h), np.uint8)
                lib().zinc_zip_proof_read(h, roots.ctypes.data, v.ctypes.data, proof.ctypes.data)
            finally:
                lib().zinc_zip_proof_free(h)
            out["zip_proof"] = dict(z_comm=roots, v=v, pcs_proof=proof)
        return out

    def spartan_prove(self, matrices, s, d, S, c, public_input, w_ccs, transcript: KeccakTranscript, field: FieldConfig,
                      prepared=None):
        """prepare_for_random_field_piop + SpartanProver::prove (prover.rs:130-161) -> SpartanProof fields + r_y."""
        return self._run(matrices, s, d, S, c, public_input, w_ccs, transcript, field, False, prepared)

    def prove(self, matrices, s, d, S, c, public_input, w_ccs, transcript: KeccakTranscript, field: FieldConfig,
              prepared=None):
        """Prover::prove (prover.rs:50-88) -> ZincProof {spartan_proof, zip_proof}."""
        return self._run(matrices, s, d, S, c, public_input, w_ccs, transcript, field, True, prepared)

    def _run_batch(self, matrices, s, d, S, c, xs, ws, transcripts, fields, with_pcs):
        B, t = len(xs), len(matrices)
        assert len(ws) == B and len(transcripts) == B and len(fields) == B
        arr, _keep = self._abi_matrices(matrices)
        masks = np.array([sum(1 << j for j in Si) for Si in S], dtype=np.uint32)
        cv = np.array(c, dtype=np.int64)
        x = [np.ascontiguousarray(v, dtype=np.int64).reshape(-1) for v in xs]
        w = [np.ascontiguousarray(v, dtype=np.int64).reshape(-1) for v in ws]
        n = max(B, 1)
        xp = (C.c_void_p * n)(*[v.ctypes.data for v in x])
        wp = (C.c_void_p * n)(*[v.ctypes.data for v in w])
        xl = (C.c_size_t * n)(*[v.size for v in x])
        wl = (C.c_size_t * n)(*[v.size for v in w])
        trs = (C.c_void_p * n)(*[tr._h for tr in transcripts])
        limbs = np.array([f.limbs for f in fields], dtype=np.uint32)
        moduli = np.zeros((n, 4), dtype=np.uint64)
        for i, f in enumerate(fields):
            moduli[i, :f.limbs] = np.asarray(f._m, dtype=np.uint64)[:f.limbs]
        total = int(limbs.sum())
        m1, m2 = np.zeros(s * (d + 2) * total, np.uint64), np.zeros(s * 3 * total, np.uint64)
        vs, ry = np.zeros(t * total, np.uint64), np.zeros(s * total, np.uint64)
        hs = (C.c_void_p * n)()
        _check(lib().zinc_prover_prove_batch(_spec_ptr(self.spec), arr, t, s, d, len(S), masks.ctypes.data, cv.ctypes.data, B, xp, xl,
                                             wp, wl, trs, moduli.ctypes.data, limbs.ctypes.data, self.device, 1 if with_pcs else 0,
                                             m1.ctypes.data, m2.ctypes.data, vs.ctypes.data, ry.ctypes.data, hs))
        out, at = [], 0
        for i, fl in enumerate(int(v) for v in limbs):
            o = dict(msgs1=m1[at * s * (d + 2):(at + fl) * s * (d + 2)].reshape(s, d + 2, fl),
                     msgs2=m2[at * s * 3:(at + fl) * s * 3].reshape(s, 3, fl),
                     V_s=vs[at * t:(at + fl) * t].reshape(t, fl), r_y=ry[at * s:(at + fl) * s].reshape(s, fl))
            at += fl
            if with_pcs:
                h = C.c_void_p(hs[i])
                try:
                    roots = np.zeros((lib().zinc_zip_proof_num_roots(h), 32), np.uint8)
                    v = np.zeros(fl, np.uint64)
                    proof = np.zeros(lib().zinc_zip_proof_len(h), np.uint8)
                    lib().zinc_zip_proof_read(h, roots.ctypes.data, v.ctypes.data, proof.ctypes.data)
                finally:
                    lib().zinc_zip_proof_free(h)
                o["zip_proof"] = dict(z_comm=roots, v=v, pcs_proof=proof)
            out.append(o)
        return out

    def spartan_prove_batch(self, matrices, s, d, S, c, xs, ws, transcripts, fields):
        """spartan_prove for B proofs of ONE circuit: xs[i], ws[i], transcripts[i], fields[i] per proof -> a list of the
        dicts spartan_prove returns; every transcript ends where spartan_prove leaves it.  From 2 proofs on (s <= 16, one
        limb count) the circuit goes up once as integers (zip_ccs_batch), the tables of all proofs are built with a launch
        count that does not depend on B and both sumchecks are one zip_sumcheck_prove_batch each; ZIP_HIP_BATCH=0, one
        proof and every other shape take the loop."""
        return self._run_batch(matrices, s, d, S, c, xs, ws, transcripts, fields, False)

    def prove_batch(self, matrices, s, d, S, c, xs, ws, transcripts, fields):
        """spartan_prove_batch, then the PCS step of every proof (ZincProver::pcs_step_batch): each proof draws its code
        from its own transcript, and from the line of min_pcs_batch on (none by default until the per-member delivery is
        measured; ZIP_HIP_PCS_MIN_BATCH=n sets one) all of them are committed in one zip_batch_commit_codes and opened in
        one zip_batch_open_eval_fields and one zip_batch_open_each; ZIP_HIP_BATCH=0, one proof, more than one proximity
        test and every other shape take the loop over the one-proof step, with the same bytes -> a list of the dicts
        prove returns."""
        return self._run_batch(matrices, s, d, S, c, xs, ws, transcripts, fields, True)

    def pcs_step_batch(self, s, zs, r_ys, transcripts, fields):
        """The PCS step of prove_batch alone (ZincProver::pcs_step_batch; tools/pcs_batch_times.py): zs[i] the z vector
        (x || 1 || w) of proof i, r_ys[i] its point [s, limbs] and transcripts[i] as spartan_prove_batch left them
        -> a list of zip_proof dicts (z_comm, v, pcs_proof)."""
        B = len(zs)
        assert len(r_ys) == B and len(transcripts) == B and len(fields) == B
        z = [np.ascontiguousarray(v, dtype=np.int64).reshape(-1) for v in zs]
        n = max(B, 1)
        zp = (C.c_void_p * n)(*[v.ctypes.data for v in z])
        zl = (C.c_size_t * n)(*[v.size for v in z])
        trs = (C.c_void_p * n)(*[tr._h for tr in transcripts])
        limbs = np.array([f.limbs for f in fields], dtype=np.uint32)
        moduli = np.zeros((n, 4), dtype=np.uint64)
        for i, f in enumerate(fields):
            moduli[i, :f.limbs] = np.asarray(f._m, dtype=np.uint64)[:f.limbs]
        ry = np.concatenate([np.ascontiguousarray(r, dtype=np.uint64).reshape(-1) for r in r_ys]) if B else np.zeros(1, np.uint64)
        assert ry.size == s * int(limbs.sum()) or not B
        hs = (C.c_void_p * n)()
        _check(lib().zinc_prover_pcs_step_batch(_spec_ptr(self.spec), s, B, zp, zl, ry.ctypes.data, trs, moduli.ctypes.data,
                                                limbs.ctypes.data, self.device, hs))
        out = []
        for i, fl in enumerate(int(v) for v in limbs):
            h = C.c_void_p(hs[i])
            try:
                roots = np.zeros((lib().zinc_zip_proof_num_roots(h), 32), np.uint8)
                v = np.zeros(fl, np.uint64)
                proof = np.zeros(lib().zinc_zip_proof_len(h), np.uint8)
                lib().zinc_zip_proof_read(h, roots.ctypes.data, v.ctypes.data, proof.ctypes.data)
            finally:
                lib().zinc_zip_proof_free(h)
            out.append(dict(z_comm=roots, v=v, pcs_proof=proof))
        return out


class ZincVerifier:
    """ZincVerifier (src/zinc/verifier.rs).  The draw_random_field check of Verifier::verify (:53-57) runs when `verify`
    is given the public input; without it the verifier takes the field it is handed.
    spec: the LinearCodeSpec of ZincVerifier::new (None: the default); it must be the prover's."""

    def __init__(self, device: int = 0, spec: "LinearCodeSpec" = None):
        self.device = device
        self.spec = spec

    def _run(self, matrices, s, d, S, c, proof, transcript, field, with_pcs, prepared, public_input=None):
        t, fl = len(matrices), field.limbs
        x = None if public_input is None else np.ascontiguousarray(public_input, dtype=np.int64).reshape(-1)
        arr, _keep = ZincProver._abi_matrices(matrices)
        masks = np.array([sum(1 << j for j in Si) for Si in S], dtype=np.uint32)
        cv = np.array(c, dtype=np.int64)
        m1 = np.ascontiguousarray(proof["msgs1"], dtype=np.uint64)
        m2 = np.ascontiguousarray(proof["msgs2"], dtype=np.uint64)
        vs = np.ascontiguousarray(proof["V_s"], dtype=np.uint64)
        assert m1.shape == (s, d + 2, fl) and m2.shape == (s, 3, fl) and vs.shape == (t, fl)
        pts = dict(rx_ry=np.zeros((2 * s, fl), np.uint64), e_y=np.zeros(fl, np.uint64), gamma=np.zeros(fl, np.uint64))
        roots = v = pp = None
        if with_pcs:
            zp = proof["zip_proof"]
            roots = np.ascontiguousarray(zp["z_comm"], dtype=np.uint8)
            v = np.ascontiguousarray(zp["v"], dtype=np.uint64)
            pp = np.ascontiguousarray(zp["pcs_proof"], dtype=np.uint8)
        _check(lib().zinc_verifier_verify_checked_spec(_spec_ptr(self.spec), x.ctypes.data if x is not None and x.size else None, x.size if x is not None else 0,
                                                  0 if x is None else 1, arr, t, s, d, len(S), masks.ctypes.data, cv.ctypes.data, transcript._h,
                                          field._m.ctypes.data, fl, self.device,
                                          prepared._h if prepared is not None else None, m1.ctypes.data, m2.ctypes.data,
                                          vs.ctypes.data, 1 if with_pcs else 0,
                                          roots.ctypes.data if with_pcs else None, roots.shape[0] if with_pcs else 0,
                                          v.ctypes.data if with_pcs else None, pp.ctypes.data if with_pcs else None,
                                          pp.size if with_pcs else 0, pts["rx_ry"].ctypes.data, pts["e_y"].ctypes.data,
                                          pts["gamma"].ctypes.data))
        return pts

    def spartan_verify(self, matrices, s, d, S, c, proof, transcript: KeccakTranscript, field: FieldConfig):
        """SpartanVerifier::verify (verifier.rs:105-139) -> VerificationPoints; raises SpartanError."""
        return self._run(matrices, s, d, S, c, proof, transcript, field, False, None)

    def verify(self, matrices, s, d, S, c, proof, transcript: KeccakTranscript, field: FieldConfig, prepared=None,
               public_input=None):
        """Verifier::verify (verifier.rs:45-76); raises SpartanError / InvalidPcsOpen.
        public_input (Statement_Z.public_input): when given, the reference's first check runs first, on the same
        transcript -- draw_random_field(public_input, transcript) must be `field`, else FieldConfigError before any
        other work (:53-57; the check is the C++ mirror's, ZincVerifier::check_field).  None: no such check, the field
        is taken as handed."""
        return self._run(matrices, s, d, S, c, proof, transcript, field, True, prepared, public_input)

    def check_field_batch(self, public_inputs, transcripts, fields):
        """The field check of Verifier::verify (:53-57) for every member of a batch (ZincVerifier::check_field_batch) ->
        a list of bools: the field drawn from public_inputs[i] on transcripts[i], at fields[i].limbs limbs, is fields[i].
        Nothing is raised for a member that fails; every transcript is left where the check of `verify` leaves it."""
        n = len(transcripts)
        assert len(public_inputs) == n and len(fields) == n
        _keep, ptrs, lens = _public_inputs(public_inputs)
        trs = (C.c_void_p * max(n, 1))(*[t._h for t in transcripts])
        limbs = np.array([f.limbs for f in fields] or [0], dtype=np.uint32)
        moduli = np.zeros((max(n, 1), 4), dtype=np.uint64)
        for i, f in enumerate(fields):
            moduli[i, :f.limbs] = np.asarray(f._m, dtype=np.uint64)[:f.limbs]
        same = np.zeros(max(n, 1), np.uint8)
        _check(lib().zinc_verifier_check_field_batch(ptrs, lens, trs, n, moduli.ctypes.data, limbs.ctypes.data, self.device,
                                                     same.ctypes.data))
        return [bool(x) for x in same[:n]]

    def verify_batch_checked(self, matrices, s, d, S, c, proofs, transcripts, fields, public_inputs):
        """verify_batch with the field check first (ZincVerifier::verify_batch_checked): check_field_batch over all
        members, verify_batch over those that passed.  A member that failed the check has a FieldConfigError in the
        returned list and its transcript where the check left it."""
        assert len(public_inputs) == len(proofs)
        return self.verify_batch(matrices, s, d, S, c, proofs, transcripts, fields, _checked_inputs=public_inputs)

    def verify_batch(self, matrices, s, d, S, c, proofs, transcripts, fields, _checked_inputs=None):
        """verify for B proofs of ONE circuit (the dicts prove_batch returns), proofs[i] on transcripts[i] in fields[i]
        (ZincVerifier::verify_batch) -> a list with None per accepted proof and, not raised, the exception object verify
        would have raised for that proof alone (SpartanError / InvalidPcsOpen) otherwise.  Every transcript ends where
        verify leaves it, for rejected proofs as well.  From the line profiles/verify_batch.md sets on (ZIP_HIP_VERIFY_MIN_BATCH=n
        moves it) the PCS part of proofs of one limb count is one zip_batch_verify_codes and the matrix MLEs one
        zip_ccs_batch_eval_matrices; otherwise, and with ZIP_HIP_BATCH=0, the loop over verify runs inside the call."""
        B, t = len(proofs), len(matrices)
        assert len(transcripts) == B and len(fields) == B
        arr, _keep = ZincProver._abi_matrices(matrices)
        masks = np.array([sum(1 << j for j in Si) for Si in S], dtype=np.uint32)
        cv = np.array(c, dtype=np.int64)
        n = max(B, 1)
        limbs = np.array([f.limbs for f in fields], dtype=np.uint32)
        moduli = np.zeros((n, 4), dtype=np.uint64)
        for i, f in enumerate(fields):
            moduli[i, :f.limbs] = np.asarray(f._m, dtype=np.uint64)[:f.limbs]

        def flat(key, shape):
            parts = []
            for p, f in zip(proofs, fields):
                a = np.ascontiguousarray(p[key], dtype=np.uint64)
                assert a.shape == shape + (f.limbs,), (key, a.shape)
                parts.append(a.reshape(-1))
            return np.concatenate(parts) if parts else np.zeros(1, np.uint64)

        m1, m2, vs = flat("msgs1", (s, d + 2)), flat("msgs2", (s, 3)), flat("V_s", (t,))
        roots = [np.ascontiguousarray(p["zip_proof"]["z_comm"], dtype=np.uint8).reshape(-1, 32) for p in proofs]
        streams = [np.ascontiguousarray(p["zip_proof"]["pcs_proof"], dtype=np.uint8).reshape(-1) for p in proofs]
        v = np.concatenate([np.ascontiguousarray(p["zip_proof"]["v"], dtype=np.uint64).reshape(-1) for p in proofs]) if B else np.zeros(1, np.uint64)
        assert v.size == int(limbs.sum()) or not B
        trs = (C.c_void_p * n)(*[tr._h for tr in transcripts])
        rp = (C.c_void_p * n)(*[r.ctypes.data for r in roots])
        rn = (C.c_size_t * n)(*[r.shape[0] for r in roots])
        pp = (C.c_void_p * n)(*[p.ctypes.data for p in streams])
        pl = (C.c_size_t * n)(*[p.size for p in streams])
        results = np.zeros(n, dtype=np.int32)
        cap = 256
        messages = C.create_string_buffer(n * cap)
        args = (_spec_ptr(self.spec), arr, t, s, d, len(S), masks.ctypes.data, cv.ctypes.data, B, trs, moduli.ctypes.data,
                limbs.ctypes.data, self.device, m1.ctypes.data, m2.ctypes.data, vs.ctypes.data, rp, rn, v.ctypes.data, pp, pl,
                results.ctypes.data, messages, cap)
        if _checked_inputs is None:
            _check(lib().zinc_verifier_verify_batch(*args))
        else:
            _keep_x, xp, xl = _public_inputs(_checked_inputs)
            _check(lib().zinc_verifier_verify_batch_checked(xp, xl, *args))
        raw = messages.raw
        return [_error(int(results[i]), raw[i * cap:(i + 1) * cap].split(b"\0", 1)[0].decode()) for i in range(B)]


class PreparedCcs:
    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        try:  # (at interpreter shutdown the module globals may already be gone)
            if getattr(self, "_h", None):
                lib().zinc_prepared_ccs_free(self._h)
                self._h = None
        except Exception:
            pass
