"""GPU: zip_sumcheck_prove_batch -- many small sumchecks, one workgroup each, in one launch (sumcheck_batch_kernel).  The
oracle gives the expected values one instance at a time; "equal" always means: the round messages, the challenges and
the sponge afterwards (st, buflen, buf[:buflen], zeros beyond) equal the oracle's, bit for bit."""
import numpy as np
import pytest

import _oracle as orc

pytestmark = pytest.mark.gpu

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503
MOD_NO_SPARE = (1 << 256) - 189
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59
STARK = (1 << 251) + 17 * (1 << 192) + 1
MOD_129_BITS = (1 << 128) + 51          # 3 limbs: the hi mask keeps 0 bits
MOD_128_NO_SPARE = (1 << 128) - 159     # 2 limbs, no spare bit
MOD_130_BITS = (1 << 129) + (1 << 64) + 1


def _lds_tail_bound(K, fl):
    """The default of ZIP_HIP_SUMCHECK_TAIL: K tables of 2^n entries in the 160 KiB of LDS of one workgroup beside ~5 KiB
    of the kernel's own (kernels_sumcheck_tail.cuh), n <= 13."""
    n = 0
    while n < 13 and (K << (n + 1)) * fl * 8 + 5 * 1024 <= 160 * 1024:
        n += 1
    return n


def _lds_rounds(K, fl, nv, knob):
    bound = _lds_tail_bound(K, fl)
    try:
        n = int(knob) if knob is not None else bound
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


class _Inst:
    """one instance: its tables, field, primed transcript -- and what the oracle makes of it (computed once)"""

    def __init__(self, cabi, modulus, fl, mles, degree, prime=b"", masks=None, coeffs=None):
        self.modulus, self.fl, self.mles, self.degree, self.prime = modulus, fl, mles, degree, prime
        self.field = cabi.make_field(modulus, fl)
        self.comb = None if masks is None else cabi.make_comb(masks, orc.field_elems(coeffs, fl))
        f = orc.make_field(modulus, fl)
        self.to = orc.new_transcript()
        if prime:
            orc.absorb(self.to, prime)
        self.state = _state_of(cabi, self.to)
        if masks is None:
            self.msgs_o, self.rand_o = orc.sumcheck_prove_product(f, mles, degree, self.to)
        else:
            self.msgs_o, self.rand_o = orc.sumcheck_prove(f, mles, degree, masks, coeffs, self.to)

    def fresh_state(self, cabi):
        to = orc.new_transcript()
        if self.prime:
            orc.absorb(to, self.prime)
        self.state = _state_of(cabi, to)
        return self.state


def _run(cabi, insts, degree=None, tables=None, knob=None):
    """one zip_sumcheck_prove_batch over `insts` against the oracle; `tables[i]`: what instance i hands over instead of
    its numpy array (device tensors); `knob`: the value ZIP_HIP_SUMCHECK_TAIL has (for the streamed-rounds count)"""
    K, nv, fl = insts[0].mles.shape[0], insts[0].mles.shape[1].bit_length() - 1, insts[0].fl
    degree = insts[0].degree if degree is None else degree
    args = [(i.mles if tables is None else tables[n], i.field, i.state, i.comb) for n, i in enumerate(insts)]
    c0 = cabi.sumcheck_batch_counts()
    msgs, rand = cabi.sumcheck_prove_batch(args, K, nv, degree)
    c1 = cabi.sumcheck_batch_counts()
    streamed = nv - _lds_rounds(K, fl, nv, knob)
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (1, len(insts), len(insts) * streamed)
    assert msgs.shape == (len(insts), nv, degree + 1, fl) and rand.shape == (len(insts), nv, fl)
    for n, i in enumerate(insts):
        assert np.array_equal(msgs[n], i.msgs_o), f"instance {n}: messages"
        assert np.array_equal(rand[n], i.rand_o), f"instance {n}: challenges"
        _assert_state_equal(i.state, i.to, f"instance {n}: sponge")
    return msgs, rand


@pytest.mark.parametrize("modulus,fl", [(BENCH_MODULUS, 4), (TEST_MODULUS_2, 2), (MOD_3LIMB, 3), (MOD_NO_SPARE, 4)])
def test_field_grid(mods, monkeypatch, modulus, fl):
    """B = 3, product of two tables: different tables, transcripts primed with 0, 7 and 135 bytes; with 4 limbs three
    different moduli in one call"""
    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    moduli = [BENCH_MODULUS, MOD_NO_SPARE, STARK] if fl == 4 else [modulus] * 3
    if modulus == MOD_NO_SPARE:
        moduli = [MOD_NO_SPARE, STARK, BENCH_MODULUS]
    insts = []
    for n, (q, p) in enumerate(zip(moduli, (0, 7, 135))):
        f = orc.make_field(q, fl)
        insts.append(_Inst(cabi, q, fl, _tables(f, fl, q, 2, 5, seed=11 + n), 2, prime=bytes(range(p))))
    _run(cabi, insts)


def test_ccs_forms_per_instance(mods, monkeypatch):
    """B = 4, K = 4, nv = 6, the forms per instance: the CCS comb in two fields and comb = NULL among combs at degree 3;
    with the three-term comb with a zero coefficient (skipped, zinc/utils.rs:80-82) in the batch, degree 4 for that call"""
    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    modulus, fl, nv = BENCH_MODULUS, 4, 6
    f = orc.make_field(modulus, fl)
    R = 1 << (64 * fl)
    masks, c = _ccs_comb(modulus, fl)
    c3 = [x * R % modulus for x in (5, 0, modulus - 7)]
    tabs = [_tables(f, fl, modulus, 4, nv, seed=40 + n) for n in range(3)]
    tabs.append(_tables(orc.make_field(STARK, fl), fl, STARK, 4, nv, seed=43))
    for degree in (3, 4):
        second = dict(masks=masks, coeffs=c) if degree == 3 else dict(masks=[0b111, 0b101], coeffs=[c3[0], c3[2]])
        insts = [
            _Inst(cabi, modulus, fl, tabs[0], degree, prime=b"sumcheck-1", masks=masks, coeffs=c),
            _Inst(cabi, modulus, fl, tabs[1], degree, prime=b"x" * 100, **second),
            _Inst(cabi, modulus, fl, tabs[2], degree),  # comb = NULL: the product of all four
            _Inst(cabi, STARK, fl, tabs[3], degree, prime=b"other field", masks=masks, coeffs=_ccs_comb(STARK, fl)[1]),
        ]
        _run(cabi, insts, degree=degree)


@pytest.mark.parametrize("modulus,fl", [(BENCH_MODULUS, 4), (TEST_MODULUS_2, 2)])
def test_every_sponge_offset_in_one_call(mods, monkeypatch, modulus, fl):
    """B = 137, instance p primed with p bytes: every block boundary, and more instances than one"""
    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    f = orc.make_field(modulus, fl)
    base = _tables(f, fl, modulus, 2, 3, seed=23)
    insts = [_Inst(cabi, modulus, fl, np.roll(base, p, axis=1).copy(), 2, prime=bytes(range(p))) for p in range(137)]
    _run(cabi, insts)


def test_more_instances_than_cus(mods, monkeypatch):
    import torch

    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    B = torch.cuda.get_device_properties(0).multi_processor_count + 3
    modulus, fl = TEST_MODULUS_2, 2
    rng = np.random.default_rng(3)
    insts = [_Inst(cabi, modulus, fl, rng.integers(0, 1 << 30, size=(1, 4, fl), dtype=np.uint64), 1, prime=bytes([n & 255]) * (n % 136))
             for n in range(B)]
    _run(cabi, insts)  # (launches + 1, instances + B: checked there)


@pytest.mark.parametrize("shape", ["product", "ccs"])
def test_one_instance_equals_the_handle(mods, monkeypatch, shape):
    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    modulus, fl, nv = BENCH_MODULUS, 4, 7
    f = orc.make_field(modulus, fl)
    if shape == "product":
        inst = _Inst(cabi, modulus, fl, _tables(f, fl, modulus, 2, nv, seed=61), 2, prime=b"one")
    else:
        masks, c = _ccs_comb(modulus, fl)
        inst = _Inst(cabi, modulus, fl, _tables(f, fl, modulus, 4, nv, seed=62), 3, prime=b"one", masks=masks, coeffs=c)
    msgs, rand = _run(cabi, [inst])
    state = inst.fresh_state(cabi)
    sc = cabi.Sumcheck(inst.mles, nv, inst.degree, inst.field, comb=inst.comb)
    m1, r1 = sc.prove(state)
    sc.free()
    assert np.array_equal(msgs[0], m1) and np.array_equal(rand[0], r1)
    _assert_state_equal(state, inst.to)


@pytest.fixture(scope="module")
def threshold_insts(mods):
    cabi, _ = mods
    modulus, fl, nv = BENCH_MODULUS, 4, 6
    f = orc.make_field(modulus, fl)
    masks, c = _ccs_comb(modulus, fl)
    return {
        "product": [_Inst(cabi, modulus, fl, _tables(f, fl, modulus, 2, nv, seed=70 + n), 2, prime=b"t" * n) for n in range(2)],
        "ccs": [_Inst(cabi, modulus, fl, _tables(f, fl, modulus, 4, nv, seed=80 + n), 3, prime=b"t" * n, masks=masks, coeffs=c)
                for n in range(2)],
    }


@pytest.mark.parametrize("tail", ["0", "1", "3", None, "13", "junk", "14", "-1"])
@pytest.mark.parametrize("shape", ["product", "ccs"])
def test_lds_threshold(mods, monkeypatch, threshold_insts, shape, tail):
    """ZIP_HIP_SUMCHECK_TAIL: every round streamed, one LDS round, LDS entered mid-way, the default, the largest value
    (cut to the bound and to nv); junk leaves the default.  streamed_rounds grows by B * (nv - min(n, bound, nv))."""
    cabi, _ = mods
    if tail is None:
        monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    else:
        monkeypatch.setenv("ZIP_HIP_SUMCHECK_TAIL", tail)
    insts = threshold_insts[shape]
    for i in insts:
        i.fresh_state(cabi)
    _run(cabi, insts, knob=tail)


@pytest.mark.parametrize("K,nv,ccs", [(4, 12, True), (2, 13, False), (2, 16, False)])
def test_default_threshold_crossed_at_real_size(mods, monkeypatch, K, nv, ccs):
    """unset knob, 4 limbs: two streamed rounds with several fold passes each above the LDS bound (K = 4: 10, K = 2: 11),
    and nv = 16, the limit"""
    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    modulus, fl = BENCH_MODULUS, 4
    assert nv > _lds_tail_bound(K, fl)
    masks, c = _ccs_comb(modulus, fl) if ccs else (None, None)
    insts = [_Inst(cabi, modulus, fl, _big_tables(fl, K, nv, seed=nv + n), 3 if ccs else 2, prime=b"big" * n, masks=masks, coeffs=c)
             for n in range(2)]
    _run(cabi, insts)


@pytest.mark.parametrize("nv", [1, 2, 3, 12])
def test_every_round_streamed(mods, monkeypatch, nv):
    """knob 0: fewer points than lanes, exactly one pass, many passes"""
    cabi, _ = mods
    monkeypatch.setenv("ZIP_HIP_SUMCHECK_TAIL", "0")
    modulus, fl = BENCH_MODULUS, 4
    insts = [_Inst(cabi, modulus, fl, _big_tables(fl, 2, nv, seed=100 + nv + n), 2, prime=b"s" * (50 * n)) for n in range(2)]
    _run(cabi, insts, knob="0")


def test_device_resident_tables_are_only_read(mods, monkeypatch):
    import torch

    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    modulus, fl, nv, K = BENCH_MODULUS, 4, 12, 2
    insts = [_Inst(cabi, modulus, fl, _big_tables(fl, K, nv, seed=200 + n), 2, prime=b"device" * n) for n in range(3)]
    m_host, r_host = _run(cabi, insts)
    dev = [[torch.from_numpy(i.mles[k].view(np.int64)).cuda() for k in range(K)] for i in insts]
    before = [[d.clone() for d in ds] for ds in dev]
    for i in insts:
        i.fresh_state(cabi)
    m_dev, r_dev = _run(cabi, insts, tables=dev)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for ds, bs in zip(dev, before) for a, b in zip(ds, bs))
    assert np.array_equal(m_host, m_dev) and np.array_equal(r_host, r_dev)


@pytest.mark.parametrize("modulus,fl", [(MOD_129_BITS, 3), (MOD_128_NO_SPARE, 2), (MOD_130_BITS, 3)])
def test_challenge_branch_edges(mods, monkeypatch, modulus, fl):
    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    f = orc.make_field(modulus, fl)
    insts = [_Inst(cabi, modulus, fl, _tables(f, fl, modulus, 3, 5, seed=5 * n + 3), 3, prime=b"sumcheck-2" * n) for n in range(3)]
    _run(cabi, insts)


def test_refused_call_changes_nothing_then_succeeds(mods, monkeypatch):
    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    modulus, fl = BENCH_MODULUS, 4
    f = orc.make_field(modulus, fl)
    insts = [_Inst(cabi, modulus, fl, _tables(f, fl, modulus, 2, 4, seed=300 + n), 2, prime=b"r" * n) for n in range(3)]
    counts = cabi.sumcheck_batch_counts()
    # buflen = 136 in the middle of the batch
    insts[1].state.buflen = 136
    before = [bytes(i.state) for i in insts]
    with pytest.raises(cabi.ZipError) as e:
        cabi.sumcheck_prove_batch([(i.mles, i.field, i.state, None) for i in insts], 2, 4, 2)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    assert [bytes(i.state) for i in insts] == before and cabi.sumcheck_batch_counts() == counts
    insts[1].fresh_state(cabi)
    # mixed limbs
    before = [bytes(i.state) for i in insts]
    with pytest.raises(cabi.ZipError) as e:
        cabi.sumcheck_prove_batch([(i.mles, cabi.make_field(TEST_MODULUS_2, 2) if n == 2 else i.field, i.state, None)
                                   for n, i in enumerate(insts)], 2, 4, 2)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    assert [bytes(i.state) for i in insts] == before and cabi.sumcheck_batch_counts() == counts
    _run(cabi, insts)  # the same batch, corrected


def test_other_counters_do_not_move(mods, monkeypatch):
    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    modulus, fl = BENCH_MODULUS, 4
    insts = [_Inst(cabi, modulus, fl, _big_tables(fl, 2, 12, seed=400 + n), 2) for n in range(2)]
    launch, grid = cabi.sumcheck_launch_counts(), cabi.sumcheck_grid_counts()
    _run(cabi, insts)
    assert cabi.sumcheck_launch_counts() == launch and cabi.sumcheck_grid_counts() == grid


def _mirror_run(cabi, pcs, monkeypatch, batch_env, mles, degree, fields, combs, primes):
    if batch_env is None:
        monkeypatch.delenv("ZIP_HIP_BATCH", raising=False)
    else:
        monkeypatch.setenv("ZIP_HIP_BATCH", batch_env)
    ts = []
    for p in primes:
        t = pcs.KeccakTranscript()
        t.absorb(p)
        ts.append(t)
    c0 = cabi.sumcheck_batch_counts()[0]
    msgs, rand = pcs.sumcheck_prove_batch(ts, mles, degree, fields, combs)
    return msgs, rand, [t.get_u64() for t in ts], cabi.sumcheck_batch_counts()[0] - c0


@pytest.mark.parametrize("shape", ["product", "ccs"])
def test_mirror_batch_equals_loop_and_oracle(mods, monkeypatch, shape):
    cabi, pcs = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    fl, nv, B = 4, 6, 3
    moduli = [BENCH_MODULUS, STARK, BENCH_MODULUS]
    K, degree = (2, 2) if shape == "product" else (4, 3)
    S = [[0, 1], [2]]
    mles = [_tables(orc.make_field(q, fl), fl, q, K, nv, seed=500 + n) for n, q in enumerate(moduli)]
    fields = [pcs.FieldConfig(q, fl) for q in moduli]
    primes = [b"mirror" * (n + 1) for n in range(B)]
    combs = None if shape == "product" else [(orc.field_elems(_ccs_comb(q, fl)[1], fl), S) for q in moduli]
    runs = {env: _mirror_run(cabi, pcs, monkeypatch, env, mles, degree, fields, combs, primes) for env in ("0", "1", None)}
    assert runs["0"][3] == 0 and runs["1"][3] == 1 and runs[None][3] == 1  # the batch counter moves on the batched path only
    for env in ("1", None):
        for a, b in zip(runs["0"][0] + runs["0"][1], runs[env][0] + runs[env][1]):
            assert np.array_equal(a, b), env
        assert runs["0"][2] == runs[env][2], env
    for n, q in enumerate(moduli):  # the loop of the one-at-a-time functions, and the oracle
        t = pcs.KeccakTranscript()
        t.absorb(primes[n])
        to = orc.new_transcript()
        orc.absorb(to, primes[n])
        f = orc.make_field(q, fl)
        if shape == "product":
            m, r = pcs.sumcheck_prove_product(t, mles[n], degree, fields[n])
            mo, ro = orc.sumcheck_prove_product(f, mles[n], degree, to)
        else:
            m, r = pcs.sumcheck_prove_ccs(t, mles[n], degree, combs[n][0], S, fields[n])
            masks, c = _ccs_comb(q, fl)
            mo, ro = orc.sumcheck_prove(f, mles[n], degree, masks, c, to)
        u_loop, u_orc = t.get_u64(), orc.lib().orc_tr_get_u64(orc.C.byref(to))
        for env in ("0", None):
            assert np.array_equal(runs[env][0][n], m) and np.array_equal(runs[env][1][n], r), (env, n)
            assert np.array_equal(runs[env][0][n], mo) and np.array_equal(runs[env][1][n], ro), (env, n)
            assert runs[env][2][n] == u_loop == u_orc, (env, n)


def test_mirror_17_variables_takes_the_loop(mods, monkeypatch):
    cabi, pcs = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    fl, nv = 4, 17
    mles = [_big_tables(fl, 2, nv, seed=600 + n) for n in range(2)]
    fields = [pcs.FieldConfig(BENCH_MODULUS, fl)] * 2
    primes = [b"seventeen", b"17"]
    msgs, rand, us, moved = _mirror_run(cabi, pcs, monkeypatch, None, mles, 2, fields, None, primes)
    assert moved == 0
    f = orc.make_field(BENCH_MODULUS, fl)
    for n in range(2):
        to = orc.new_transcript()
        orc.absorb(to, primes[n])
        mo, ro = orc.sumcheck_prove_product(f, mles[n], 2, to)
        assert np.array_equal(msgs[n], mo) and np.array_equal(rand[n], ro)
        assert us[n] == orc.lib().orc_tr_get_u64(orc.C.byref(to))


def test_mirror_mixed_limbs_takes_the_loop(mods, monkeypatch):
    cabi, pcs = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    specs = [(BENCH_MODULUS, 4), (TEST_MODULUS_2, 2)]
    nv = 4
    mles = [_tables(orc.make_field(q, fl), fl, q, 2, nv, seed=700 + n) for n, (q, fl) in enumerate(specs)]
    fields = [pcs.FieldConfig(q, fl) for q, fl in specs]
    primes = [b"mixed", b"limbs"]
    msgs, rand, us, moved = _mirror_run(cabi, pcs, monkeypatch, "1", mles, 2, fields, None, primes)
    assert moved == 0
    for n, (q, fl) in enumerate(specs):
        to = orc.new_transcript()
        orc.absorb(to, primes[n])
        mo, ro = orc.sumcheck_prove_product(orc.make_field(q, fl), mles[n], 2, to)
        assert np.array_equal(msgs[n], mo) and np.array_equal(rand[n], ro)
        assert us[n] == orc.lib().orc_tr_get_u64(orc.C.byref(to))


def test_mirror_line_small_batches_take_the_loop(mods, monkeypatch):
    """where one launch does not beat the loop (profiles/sumcheck_batch.md) the mirror loops: at 2^13 two instances, and
    three are one batch call; the bytes are the oracle's either way"""
    cabi, pcs = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    fl, nv = 4, 13
    mles = [_big_tables(fl, 2, nv, seed=800 + n) for n in range(3)]
    primes = [b"line" * (n + 1) for n in range(3)]
    f = orc.make_field(BENCH_MODULUS, fl)
    want = []
    for n in range(3):
        to = orc.new_transcript()
        orc.absorb(to, primes[n])
        mo, ro = orc.sumcheck_prove_product(f, mles[n], 2, to)
        want.append((mo, ro, orc.lib().orc_tr_get_u64(orc.C.byref(to))))
    for B, batched in ((2, 0), (3, 1)):
        fields = [pcs.FieldConfig(BENCH_MODULUS, fl)] * B
        msgs, rand, us, moved = _mirror_run(cabi, pcs, monkeypatch, None, mles[:B], 2, fields, None, primes[:B])
        assert moved == batched, B
        for n in range(B):
            assert np.array_equal(msgs[n], want[n][0]) and np.array_equal(rand[n], want[n][1]) and us[n] == want[n][2], (B, n)
