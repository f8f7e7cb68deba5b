"""GPU: zip_sumcheck_prove -- MLSumcheck::prove_as_subprotocol in one call, the Keccak transcript inside the library and,
for the tail of the rounds, on the device (sumcheck_tail_kernel).  "Equal" always means: the round messages, the
challenges and the transcript afterwards (st, buflen, buf[:buflen]) equal the oracle's, bit for bit."""
import os

import numpy as np
import pytest

import _ccs
import _oracle as orc

pytestmark = pytest.mark.gpu

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503
MOD_NO_SPARE = (1 << 256) - 189
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59
# the edges of get_challenge's branches (the prover never inverts: the moduli need not be prime)
MOD_129_BITS = (1 << 128) + 51          # 3 limbs: the hi mask keeps 0 bits
MOD_128_NO_SPARE = (1 << 128) - 159     # 2 limbs, no spare bit
MOD_130_BITS = (1 << 129) + (1 << 64) + 1
Q192 = 312829638388039969874974628075306023441  # zinc/tests.rs:28

GRID_FIELDS = [(BENCH_MODULUS, 4), (TEST_MODULUS_2, 2), (MOD_NO_SPARE, 4), (MOD_3LIMB, 3)]


def _lds_tail_bound(K, fl):
    """The default of ZIP_HIP_SUMCHECK_TAIL: the tail kernel keeps K tables of 2^n entries in the 160 KiB of LDS of one
    workgroup beside ~5 KiB of its own (kernels_sumcheck_tail.cuh), n <= 13."""
    n = 0
    while n < 13 and (K << (n + 1)) * fl * 8 + 5 * 1024 <= 160 * 1024:
        n += 1
    return n


def _expected_tail_rounds(K, fl, nv):
    """How many rounds zip_sumcheck_prove gives to the tail kernel: ZIP_HIP_SUMCHECK_TAIL when it is a number in 0..13,
    else the default; never more than fits the LDS, never more than there are rounds."""
    bound = _lds_tail_bound(K, fl)
    knob = os.environ.get("ZIP_HIP_SUMCHECK_TAIL", "")
    try:
        n = int(knob)
    except ValueError:
        n = bound
    if not 0 <= n <= 13:
        n = bound
    return min(n, bound, nv)


@pytest.fixture(scope="module")
def mods():
    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, pcs


def _tables(f, fl, modulus, K, nv, seed):
    """K tables of 2^nv canonical field elements (Montgomery limbs): the witness-like one from i64, the rest random"""
    rng = np.random.default_rng(seed)
    n = 1 << nv
    out = np.zeros((K, n, fl), dtype=np.uint64)
    for k in range(K):
        if k == K - 1:
            w = orc.splitmix64(seed + k, n)
            for i in range(n):
                out[k, i] = orc.int_to_limbs(orc.field_from_i64(f, int(w[i])), fl)
        else:
            vals = [int.from_bytes(rng.bytes(40), "little") % modulus for _ in range(n)]
            out[k] = orc.field_elems(vals, fl)
    return out


def _big_tables(fl, K, nv, seed):
    """canonical residues well below the 4-limb / 3-limb test moduli, as raw Montgomery limbs (fast for large nv)"""
    rng = np.random.default_rng(seed)
    mles = rng.integers(0, 1 << 62, size=(K, 1 << nv, fl), dtype=np.uint64)
    mles[..., fl - 1] >>= np.uint64(6 if fl == 4 else 4)
    return mles


def _ccs_comb(modulus, fl):
    R = 1 << (64 * fl)
    return [0b011, 0b100], [1 * R % modulus, (modulus - 1) * R % modulus]


def _state_of(cabi, to):
    return cabi.KeccakState.make(st=[int(w) for w in to.st], buf=bytes(to.buf[: to.buflen]))


def _assert_state_equal(state, to, what=""):
    assert [int(w) for w in state.st] == [int(w) for w in to.st], what
    assert state.buflen == to.buflen, what
    assert state.pending() == bytes(to.buf[: to.buflen]), what
    assert not any(state.buf[state.buflen:]), what  # zero beyond buflen on output


def _check(cabi, modulus, fl, mles, degree, prime=b"", masks=None, coeffs=None, tables=None, what=""):
    """One zip_sumcheck_prove against the oracle's prover from the same primed transcript.  `tables`: what the handle
    gets instead of the numpy array (device tensors)."""
    f = orc.make_field(modulus, fl)
    nv = mles.shape[1].bit_length() - 1
    to = orc.new_transcript()
    if prime:
        orc.absorb(to, prime)
    state = _state_of(cabi, to)
    if masks is None:
        msgs_o, rand_o = orc.sumcheck_prove_product(f, mles, degree, to)
        comb = None
    else:
        msgs_o, rand_o = orc.sumcheck_prove(f, mles, degree, masks, coeffs, to)
        comb = cabi.make_comb(masks, orc.field_elems(coeffs, fl))
    sc = cabi.Sumcheck(mles if tables is None else tables, nv, degree, cabi.make_field(modulus, fl), comb=comb)
    rounds0, tails0 = cabi.sumcheck_launch_counts()
    msgs, rand = sc.prove(state)
    rounds1, tails1 = cabi.sumcheck_launch_counts()
    # every path gives the same bytes: which one ran is read from the launch counts
    n_tail = _expected_tail_rounds(mles.shape[0], fl, nv)
    assert tails1 - tails0 == (1 if n_tail else 0), what
    assert rounds1 - rounds0 == nv - n_tail, what
    assert np.array_equal(msgs, msgs_o), what
    assert np.array_equal(rand, rand_o), what
    _assert_state_equal(state, to, what)
    with pytest.raises(cabi.ZipError, match="not active"):  # the handle is finished (prover.rs:91-93)
        sc.round(rand_o[-1])
    sc.free()


@pytest.mark.parametrize("modulus,fl", GRID_FIELDS)
@pytest.mark.parametrize("K,degree,nv", [(2, 2, 10), (1, 1, 3), (3, 3, 7), (2, 3, 1), (4, 4, 5), (2, 2, 2)])
def test_product_grid(mods, modulus, fl, K, degree, nv):
    cabi, _ = mods
    f = orc.make_field(modulus, fl)
    _check(cabi, modulus, fl, _tables(f, fl, modulus, K, nv, seed=nv * 7 + K), degree, prime=b"sumcheck-2")


@pytest.mark.parametrize("modulus,fl", [(BENCH_MODULUS, 4), (TEST_MODULUS_2, 2)])
def test_every_sponge_offset(mods, modulus, fl):
    """The transcript primed with p bytes for every p in 0..136: each block boundary falls inside every kind of absorbed
    piece (tags, modulus, values, the digest of get_challenge) at least once."""
    cabi, _ = mods
    f = orc.make_field(modulus, fl)
    mles = _tables(f, fl, modulus, 2, 3, seed=23)
    for p in range(137):
        _check(cabi, modulus, fl, mles, 2, prime=bytes(range(p)), what=f"offset {p}")


@pytest.mark.parametrize("modulus,fl", [(MOD_129_BITS, 3), (MOD_128_NO_SPARE, 2), (MOD_130_BITS, 3)])
@pytest.mark.parametrize("K,degree,nv", [(2, 2, 3), (3, 3, 7)])
def test_challenge_branch_edges(mods, modulus, fl, K, degree, nv):
    cabi, _ = mods
    f = orc.make_field(modulus, fl)
    _check(cabi, modulus, fl, _tables(f, fl, modulus, K, nv, seed=nv * 5 + K), degree, prime=b"sumcheck-2")


@pytest.mark.parametrize("modulus,fl", [(BENCH_MODULUS, 4), (TEST_MODULUS_2, 2), (MOD_3LIMB, 3)])
@pytest.mark.parametrize("nv", [1, 6, 11])
def test_ccs_combination(mods, modulus, fl, nv):
    """(M0 * M1 - M2) * eq, degree 3 (zinc/utils.rs:77-94)"""
    cabi, _ = mods
    f = orc.make_field(modulus, fl)
    masks, c = _ccs_comb(modulus, fl)
    _check(cabi, modulus, fl, _tables(f, fl, modulus, 4, nv, seed=nv + 40), 3, prime=b"sumcheck-1", masks=masks, coeffs=c)


def test_ccs_general_terms_and_zero_coefficient(mods):
    """three terms over three MLEs + eq, one coefficient zero (skipped, zinc/utils.rs:80-82), degree 4"""
    cabi, _ = mods
    modulus, fl, nv = BENCH_MODULUS, 4, 7
    f = orc.make_field(modulus, fl)
    R = 1 << (64 * fl)
    c = [x * R % modulus for x in (5, 0, modulus - 7)]
    _check(cabi, modulus, fl, _tables(f, fl, modulus, 4, nv, seed=9), 4, masks=[0b111, 0b101], coeffs=[c[0], c[2]])


@pytest.mark.parametrize("tail", ["0", "1", "3", None, "13"])
@pytest.mark.parametrize("shape", ["product", "ccs"])
def test_tail_boundaries(mods, monkeypatch, shape, tail):
    """ZIP_HIP_SUMCHECK_TAIL: no tail kernel, a one-round tail, a tail entered mid-way, the default (as much as fits the
    LDS) and the largest accepted value (clamped to what fits), two rounds above the default bound."""
    cabi, _ = mods
    if tail is None:
        monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    else:
        monkeypatch.setenv("ZIP_HIP_SUMCHECK_TAIL", tail)
    modulus, fl = BENCH_MODULUS, 4
    if shape == "product":
        nv = _lds_tail_bound(2, fl) + 2
        _check(cabi, modulus, fl, _big_tables(fl, 2, nv, seed=71), 2, prime=b"tail")
    else:
        nv = _lds_tail_bound(4, fl) + 2
        masks, c = _ccs_comb(modulus, fl)
        _check(cabi, modulus, fl, _big_tables(fl, 4, nv, seed=72), 3, prime=b"tail", masks=masks, coeffs=c)


@pytest.mark.parametrize("tail", ["junk", "14", "-1"])
def test_tail_knob_out_of_range_leaves_the_default(mods, monkeypatch, tail):
    cabi, _ = mods
    monkeypatch.setenv("ZIP_HIP_SUMCHECK_TAIL", tail)
    _check(cabi, BENCH_MODULUS, 4, _big_tables(4, 2, 12, seed=73), 2)


@pytest.mark.parametrize("shape", ["product", "ccs"])
@pytest.mark.parametrize("nv", [15, 17])
def test_rounds_above_the_tail(mods, shape, nv):
    """nv = 15: the last workgroup folds the partials of every large round; nv = 17: more than 64 workgroups in the
    first rounds, sumcheck_reduce_kernel folds them."""
    cabi, _ = mods
    modulus, fl = BENCH_MODULUS, 4
    if shape == "product":
        _check(cabi, modulus, fl, _big_tables(fl, 2, nv, seed=nv), 2)
    else:
        masks, c = _ccs_comb(modulus, fl)
        _check(cabi, modulus, fl, _big_tables(fl, 4, nv, seed=nv + 1), 3, masks=masks, coeffs=c)


def test_device_resident_tables_2pow20_are_only_read(mods):
    import torch  # (no importorskip: on the GPU box this case does not skip)

    cabi, _ = mods
    nv, fl, K = 20, 4, 2
    mles = _big_tables(fl, K, nv, seed=5)
    dev = [torch.from_numpy(mles[k].view(np.int64)).cuda() for k in range(K)]
    before = [d.clone() for d in dev]
    _check(cabi, BENCH_MODULUS, fl, mles, 2, prime=b"device", tables=dev)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(dev, before))


@pytest.mark.parametrize("modulus,fl", GRID_FIELDS)
def test_one_variable(mods, modulus, fl):
    """nv = 1: the only round is the tail's first: no fold at all"""
    cabi, _ = mods
    f = orc.make_field(modulus, fl)
    _check(cabi, modulus, fl, _tables(f, fl, modulus, 3, 1, seed=31), 3, prime=b"one")


@pytest.mark.parametrize("quad", ["0", "2"])
@pytest.mark.parametrize("degree", [2, 3])
def test_quad_knob(mods, monkeypatch, quad, degree):
    cabi, _ = mods
    monkeypatch.setenv("ZIP_HIP_SUMCHECK_QUAD", quad)
    _check(cabi, BENCH_MODULUS, 4, _big_tables(4, 2, 14, seed=14 + degree), degree, prime=b"quad")


def test_usage_errors(mods):
    cabi, _ = mods
    modulus, fl = BENCH_MODULUS, 4
    f = orc.make_field(modulus, fl)
    field = cabi.make_field(modulus, fl)
    mles = _tables(f, fl, modulus, 2, 4, seed=3)
    to = orc.new_transcript()
    msgs_o, rand_o = orc.sumcheck_prove_product(f, mles, 2, to)
    L = cabi.lib()
    out_m, out_r = np.zeros((4, 3, fl), np.uint64), np.zeros((4, fl), np.uint64)

    sc = cabi.Sumcheck(mles, 4, 2, field)
    st = cabi.KeccakState.make()
    assert L.zip_sumcheck_prove(None, cabi.C.byref(st), out_m.ctypes.data, out_r.ctypes.data) == cabi.ZIP_ERR_NULL
    assert L.zip_sumcheck_prove(sc._h, None, out_m.ctypes.data, out_r.ctypes.data) == cabi.ZIP_ERR_NULL
    assert L.zip_sumcheck_prove(sc._h, cabi.C.byref(st), None, out_r.ctypes.data) == cabi.ZIP_ERR_NULL
    assert L.zip_sumcheck_prove(sc._h, cabi.C.byref(st), out_m.ctypes.data, None) == cabi.ZIP_ERR_NULL
    bad = cabi.KeccakState.make()
    bad.buflen = 136
    with pytest.raises(cabi.ZipError, match="136") as e:
        sc.prove(bad)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    # none of these reached the device or used the handle up
    msgs, rand = sc.prove(st)
    assert np.array_equal(msgs, msgs_o) and np.array_equal(rand, rand_o)
    with pytest.raises(cabi.ZipError, match="already") as e:  # a second zip_sumcheck_prove
        sc.prove(cabi.KeccakState.make())
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    with pytest.raises(cabi.ZipError, match="not active"):
        sc.round(rand_o[-1])
    sc.free()

    # a handle that played a round refuses prove() and still finishes its rounds one by one
    sc = cabi.Sumcheck(mles, 4, 2, field)
    assert np.array_equal(sc.round(), msgs_o[0])
    with pytest.raises(cabi.ZipError, match="fresh") as e:
        sc.prove(cabi.KeccakState.make())
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    for i in range(1, 4):
        assert np.array_equal(sc.round(rand_o[i - 1]), msgs_o[i]), i
    sc.free()

    # a round in flight
    sc = cabi.Sumcheck(mles, 4, 2, field)
    assert L.zip_sumcheck_round_begin(sc._h, None) == 0
    with pytest.raises(cabi.ZipError, match="fresh"):
        sc.prove(cabi.KeccakState.make())
    ev = np.zeros((3, fl), np.uint64)
    assert L.zip_sumcheck_round_end(sc._h, ev.ctypes.data) == 0
    assert np.array_equal(ev, msgs_o[0])
    sc.free()


def _mirror(pcs, monkeypatch, onecall, fn):
    if onecall is None:
        monkeypatch.delenv("ZIP_HIP_SUMCHECK_ONECALL", raising=False)
    else:
        monkeypatch.setenv("ZIP_HIP_SUMCHECK_ONECALL", onecall)
    from zinc_amd import cabi

    t = pcs.KeccakTranscript()
    t.absorb(b"mirror")
    tails0 = cabi.sumcheck_launch_counts()[1]
    out = fn(t)
    tails = cabi.sumcheck_launch_counts()[1] - tails0
    if onecall == "1":  # zip_sumcheck_prove, whose default plays the last rounds in the tail kernel
        assert tails >= 1
    else:               # the per-round loop never launches it
        assert tails == 0
    return out, t.get_u64()


@pytest.mark.parametrize("modulus,fl", [(BENCH_MODULUS, 4), (MOD_3LIMB, 3), (TEST_MODULUS_2, 2)])
def test_mirror_one_call_equals_per_round(mods, monkeypatch, modulus, fl):
    """ZIP_HIP_SUMCHECK_ONECALL=1 (one zip_sumcheck_prove call), =0 and unset (the per-round loop) give the same proof"""
    _, pcs = mods
    f = orc.make_field(modulus, fl)
    field = pcs.FieldConfig(modulus, fl)
    mles = _tables(f, fl, modulus, 2, 9, seed=90)
    (m0, r0), u0 = _mirror(pcs, monkeypatch, "0", lambda t: pcs.sumcheck_prove_product(t, mles, 2, field))
    (m1, r1), u1 = _mirror(pcs, monkeypatch, "1", lambda t: pcs.sumcheck_prove_product(t, mles, 2, field))
    (m2, r2), u2 = _mirror(pcs, monkeypatch, None, lambda t: pcs.sumcheck_prove_product(t, mles, 2, field))
    assert np.array_equal(m0, m1) and np.array_equal(r0, r1) and u0 == u1
    assert np.array_equal(m0, m2) and np.array_equal(r0, r2) and u0 == u2
    to = orc.new_transcript()
    orc.absorb(to, b"mirror")
    msgs_o, rand_o = orc.sumcheck_prove_product(f, mles, 2, to)
    assert np.array_equal(m1, msgs_o) and np.array_equal(r1, rand_o) and u1 == orc.lib().orc_tr_get_u64(orc.C.byref(to))

    mles = _tables(f, fl, modulus, 4, 8, seed=91)
    _, c = _ccs_comb(modulus, fl)
    S = [[0, 1], [2]]
    ccs = lambda t: pcs.sumcheck_prove_ccs(t, mles, 3, orc.field_elems(c, fl), S, field)  # noqa: E731
    (m0, r0), u0 = _mirror(pcs, monkeypatch, "0", ccs)
    (m1, r1), u1 = _mirror(pcs, monkeypatch, "1", ccs)
    (m2, r2), u2 = _mirror(pcs, monkeypatch, None, ccs)
    assert np.array_equal(m0, m1) and np.array_equal(r0, r1) and u0 == u1
    assert np.array_equal(m0, m2) and np.array_equal(r0, r2) and u0 == u2


def _flat(x):
    if isinstance(x, dict):
        return {k: _flat(v) for k, v in x.items()}
    return np.asarray(x).tobytes()


@pytest.mark.parametrize("name", ["vitalik", "dummy1k"])
def test_zinc_prover_bytes_under_both_settings(mods, monkeypatch, name):
    """ZincProver (both sumchecks of spartan_prove through the mirror): identical proofs with the per-round loop and
    with the one-call path, and the same transcript afterwards."""
    _, pcs = mods
    inst = _ccs.vitalik_ccs(3) if name == "vitalik" else _ccs.dummy_ccs_from_len(1 << 10, seed=77)
    field = pcs.FieldConfig(Q192, 3)
    x, w = inst.z[:1], inst.z[2:]

    def run(t):
        prover = pcs.ZincProver()
        fn = prover.spartan_prove if name == "vitalik" else prover.prove
        return fn(inst.matrices, inst.s, inst.d, inst.S, inst.c, x, w, t, field)

    p0, u0 = _mirror(pcs, monkeypatch, "0", run)
    p1, u1 = _mirror(pcs, monkeypatch, "1", run)
    p2, u2 = _mirror(pcs, monkeypatch, None, run)
    assert _flat(p0) == _flat(p1) == _flat(p2) and u0 == u1 == u2
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_ONECALL", raising=False)
    to = orc.new_transcript()
    orc.absorb(to, b"mirror")
    want = orc.Ccs(inst).spartan_prove(orc.make_field(Q192, 3), to)
    for key in ("msgs1", "msgs2", "V_s", "r_y"):
        assert np.array_equal(p1[key], want[key]), key
