"""R1CS over the fields of the any-modulus path (csrc/device/r1cs_generic_kernels.hpp): even characteristics, the rings
Z / 2^k and characteristics wider than 512 bits.  The reference's ToR1CSConverter works on BigUint
(rust/src/consumers/to_r1cs.rs:93-393) and converts a relation over any modulus; with use_correction every call gets an
integer quotient wire, whatever the modulus.

CPU tier: rows from the tape against the test-side restatement of the converter and the oracle's wire values, a
caller's CSR on such a field, the kernels' arithmetic on the host against Python integers (255-term combinations of
p - 1, the exact division of the quotient wires), the kernels' resources, and the refusals that stay.  GPU tier: the
same on the card, bit-exact against Python integers or the oracle."""
import random
import re

import numpy as np
import pytest

import r1cs_ref
from helpers import batch_arrays, oracle_lane
from random_circuits import Gen
import zkinterface_ir_amd as zk
from zkinterface_ir_amd import sieve_writer as sw
from zkinterface_ir_amd import workloads


def _odd(bits, seed):
    return random.Random(seed).getrandbits(bits) | (1 << (bits - 1)) | 1


ODD600 = _odd(600, 1)
ODD1024 = _odd(1024, 2)
# even, powers of 2^32, 2^64 - 2, eight full words, wider than 512 bits (prime, odd composite), the width limit
ROW_MODULI = [6, 2 ** 32, 2 ** 64, 2 ** 64 - 2, 2 ** 256 - 2, 2 ** 521 - 1, ODD600, 2 ** 4096 - 1]
NO_VAR = 2 ** 64 - 1


def _width(p):
    return 8 * ((p.bit_length() + 63) // 64)


def _le(x, width):
    return int(x).to_bytes(width, 'little')


def _gen(p, seed):
    g = Gen(seed, p, False, switches=p.bit_length() <= 64)
    rel, mod_le = g.relation()
    return g, rel, mod_le


def _wire_values(rows, kinds, a, b, consts, p, ref_var_of, vals, use_correction):
    """variable -> value from the oracle's trace values (the assignment the converter would emit), quotient wires included"""
    w = {0: 1}
    value_ops = [i for i, k in enumerate(kinds) if int(k) != 9]
    for t, i in enumerate(value_ops[:len(vals)]):
        w[ref_var_of[i]] = vals[t]
    if use_correction:
        for i in value_ops[:len(vals)]:   # (to_r1cs.rs:183-185,235-237)
            k = int(kinds[i])
            if k in (1, 2, 3, 4):
                x = w[ref_var_of[int(a[i])]]
                y = w[ref_var_of[int(b[i])]] if k in (1, 2) else int.from_bytes(consts[int(b[i])], 'little')
                w[ref_var_of[i] + 1] = ((x + y) if k in (1, 3) else (x * y)) // p
    return w


# ---- CPU tier ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('use_correction', [False, True])
@pytest.mark.parametrize('p', ROW_MODULI)
def test_rows_from_the_tape_over_any_modulus(p, use_correction):
    """the rows of the converter rules over a canonical-residue field, and the oracle's wire values satisfy them: modulo p
    without quotient wires, exactly with them; the one exception is the row of a failing assert"""
    g, rel, mod_le = _gen(p, 900 + p.bit_length())
    ev = zk.Evaluator()
    ev.declare_inputs(g.n_inst, g.n_wit)
    ev.ingest_message(rel)
    assert ev.host_violations() == []
    assert ev.field_representation(0) == 2
    ev.r1cs_from_tape(use_correction)
    rows, var_of_op = ev.r1cs_export()
    kinds, a, b = ev.tape()
    consts = ev.constants()
    ref_rows, ref_var_of = r1cs_ref.rows_from_tape(kinds, a, b, consts, p, use_correction)
    assert rows == ref_rows
    assert [None if int(v) == NO_VAR else int(v) for v in var_of_op] == ref_var_of
    assert ev.r1cs_info()['rows'] == sum(1 for k in kinds if int(k) in (1, 2, 3, 4, 9))
    rows_i, rows_w = g.lane_inputs(4, 77)
    for lane in range(4):
        ref = oracle_lane(mod_le, rows_i[lane], rows_w[lane], [rel], _width(p))
        w = _wire_values(rows, kinds, a, b, consts, p, ref_var_of, ref.trace_values(), use_correction)
        bad = []
        for r, (A, B, C) in enumerate(rows):
            if not all(v in w for v, _ in A + B + C):
                break   # the oracle stopped at the first failing assert
            lhs = r1cs_ref.lincomb(A, w) * r1cs_ref.lincomb(B, w)
            rhs = r1cs_ref.lincomb(C, w)
            if (lhs != rhs) if use_correction else ((lhs - rhs) % p != 0):
                bad.append(r)
        if ref.violations:
            assert len(bad) == 1 and rows[bad[0]][2] == [(0, 0)], (p, lane, bad)
        else:
            assert bad == [], (p, lane)


def _csr_session(p, classes=None, M=12):
    wl = workloads.R1csSynthetic(M=M, n_base=8, n_coefs=10, seed=3, p=p)
    ev = zk.Evaluator()
    if classes is not None:
        ev.set_option('r1cs_coef_classes', classes)
    ev.declare_inputs(0, wl.n_witness)
    ev.ingest_message(wl.base_relation())
    ev.finalize(retain_all=True)
    return ev, wl


@pytest.mark.parametrize('p', [2 ** 64, 2 ** 256 - 2, 2 ** 521 - 1])
def test_load_csr_on_a_canonical_field(p):
    """a caller's CSR is accepted over such a field; every combination is of class full there, whatever the option says
    (the unit / small classes are a form of the Montgomery row kernel)"""
    for classes in ('1', '0'):
        ev, wl = _csr_session(p, classes)
        assert ev.field_representation(0) == 2
        row_ptr, tv, tc, cb = wl.csr()
        ev.r1cs_load_csr(row_ptr, tv, tc, cb, wl.width, wl.M)
        cc = ev.r1cs_class_counts()
        assert cc['unit'] == 0 and cc['small'] == 0 and cc['full'] == 3 * (wl.M + 1), (classes, cc)
        assert ev.r1cs_info()['rows'] == wl.M + 1


# moduli whose top word is 0xFFFFFFFF, a wide one, powers of two (one word, several words, the largest)
BOUND_MODULI = [2 ** 256 - 2, 2 ** 4096 - 1, 2 ** 521 - 1, 2 ** 64 - 2, 2 ** 32, 2 ** 64, 2 ** 96, 2 ** 256, 2 ** 4095, 6]


@pytest.mark.parametrize('p', BOUND_MODULI)
def test_combination_arithmetic_against_python_integers(p):
    """the row kernel's combination (one Barrett reduction per product, one conditional subtraction per sum) on the host:
    255 terms of coefficient and value p - 1 -- a sum no lazy reduction could hold below Barrett's bound -- and random ones"""
    n = 255
    assert zk.r1cs_generic_selftest(p, 'lincomb', [p - 1] * n, [p - 1] * n) == n * (p - 1) ** 2 % p
    assert zk.r1cs_generic_selftest(p, 'lincomb', [p - 1] * n) == n * (p - 1) % p
    rnd = random.Random(p.bit_length())
    for k in (1, 2, 3, 17):
        xs = [rnd.choice([0, 1, p - 1, rnd.randrange(p)]) for _ in range(k)]
        ys = [rnd.choice([1, p - 1, rnd.randrange(p)]) for _ in range(k)]
        assert zk.r1cs_generic_selftest(p, 'lincomb', xs, ys) == sum(x * y for x, y in zip(xs, ys)) % p
        assert zk.r1cs_generic_selftest(p, 'lincomb', xs) == sum(xs) % p
    assert zk.r1cs_generic_selftest(p, 'lincomb', []) == 0


# odd (prime, composite, wide), even (2^s * m, m odd > 1, s from 1 to past a word), powers of two
QUOTIENT_MODULI = [2 ** 521 - 1, ODD600, ODD1024, 2 ** 4096 - 1, 6, 2 ** 64 - 2, 2 ** 256 - 2, 3 * 2 ** 40, 5 * 2 ** 100,
                   (2 ** 61 - 1) * 2 ** 33, ODD600 * 4, 2 ** 32, 2 ** 64, 2 ** 96, 2 ** 1000, 2 ** 4095]


@pytest.mark.parametrize('p', QUOTIENT_MODULI)
def test_quotient_arithmetic_against_python_integers(p):
    """q = (a op b - out) / p with p = 2^s * m: a shift by s, then a product with m^-1 mod 2^(32 nwords); b may be a raw
    constant >= p (up to the field's whole width)"""
    rnd = random.Random(p.bit_length() + 5)
    top = 2 ** (8 * _width(p)) - 1
    cases = [(p - 1, p - 1), (0, 0), (p - 1, top), (1, top), (p - 1, p), (p - 1, 2 * p + 1 if 2 * p + 1 <= top else p)]
    cases += [(rnd.randrange(p), rnd.randrange(p)) for _ in range(4)] + [(rnd.randrange(p), rnd.randrange(p, top + 1)) for _ in range(4)]
    for x, y in cases:
        for op, full in (('add_quotient', x + y), ('mul_quotient', x * y)):
            got = zk.r1cs_generic_selftest(p, op, x, y, full % p)
            assert got == full // p, (p, op, x, y)


def test_kernel_resources_of_the_r1cs_instantiations():
    """up to eight words of characteristic the word counts are known at compile time: everything in registers; wider ones
    run the capacity classes with scratch memory bounded by the class"""
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import kernel_resources
    res = kernel_resources.resources('kernels_r1cs_generic.hip')
    small, caps, corr = {}, {}, {}
    for name, k in res.items():
        m = re.search(r'r1cs_generic_row_kernel<(\d+), (\d+), (true|false)>', name)
        if m and int(m.group(2)):
            small[(int(m.group(2)), m.group(3))] = k
        elif m:
            caps[(int(m.group(1)), m.group(3))] = k
        m = re.search(r'r1cs_generic_correction_kernel<(\d+)>', name)
        if m:
            corr[int(m.group(1))] = k
    assert sorted(small) == [(kc, a) for kc in range(1, 9) for a in ('false', 'true')]
    for key, k in small.items():
        assert k['scratch'] == 0 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['agprs'] == 0, (key, k)
        assert k['occupancy'] >= 3, (key, k)
    assert sorted(caps) == [(c, a) for c in (16, 32, 64, 128) for a in ('false', 'true')]
    for (cap, _), k in caps.items():
        assert k['vgprs'] + k['agprs'] <= 512 and k['occupancy'] >= 1, (cap, k)
        assert k['scratch'] <= 40 * cap, (cap, k)
    assert sorted(corr) == [8, 16, 32, 64, 128]
    for cap, k in corr.items():
        assert k['scratch'] <= 40 * cap, (cap, k)
    assert 'zkgpu::dump_generic_kernel' not in res   # (kernels_generic.hip's)


def test_the_refusals_that_stay():
    """a session whose field changes between Relation messages, and GF(2) (bit-packed wires)"""
    msgs = [sw.write_relation(sw.int_to_le(101), 'arithmetic', 'simple', [], [('witness', 0), ('witness', 1), ('mul', 2, 0, 1), ('free', 1, 1)]),
            sw.write_relation(sw.int_to_le(2 ** 64), 'arithmetic', 'simple', [], [('instance', 3), ('mulc', 4, 3, sw.int_to_le(2 ** 64 - 1)),
                                                                                 ('add', 5, 2, 4), ('assert_zero', 5), ('free', 0, 5)])]
    ev = zk.Evaluator()
    ev.declare_inputs(1, 2)
    for m in msgs:
        ev.ingest_message(m)
    assert ev.n_field_segments == 2
    with pytest.raises(zk.ZkGpuError, match='field characteristic changes'):
        ev.r1cs_from_tape()
    ev = zk.Evaluator()
    ev.declare_inputs(0, 2)
    ev.ingest_message(sw.write_relation(sw.int_to_le(2), 'boolean', 'simple', [], [('witness', 0), ('witness', 1), ('and', 2, 0, 1),
                                                                                 ('assert_zero', 2)]))
    with pytest.raises(zk.ZkGpuError, match='GF\\(2\\)'):
        ev.r1cs_from_tape()


# ---- GPU tier ------------------------------------------------------------------------------------------------------------

def _checked_relation(p):
    """e == (c1 * x * y + c2 + x)^2 with c1 = p - 1 and c2 = p // 3: add, multiply, add_constant, mul_constant"""
    c1, c2 = p - 1, p // 3
    gates = [('instance', 0), ('witness', 1), ('witness', 2), ('mul', 3, 1, 2), ('mulc', 4, 3, sw.int_to_le(c1)),
             ('addc', 5, 4, sw.int_to_le(c2)), ('add', 6, 5, 1), ('mul', 7, 6, 6), ('mulc', 8, 0, sw.int_to_le(p - 1)),
             ('add', 9, 7, 8), ('assert_zero', 9)]
    rel = sw.write_relation(sw.int_to_le(p), 'arithmetic', 'simple', [], gates)

    def lanes(n, seed):
        rng = random.Random(seed)
        rows_i, rows_w = [], []
        for lane in range(n):
            x, y = rng.choice([0, 1, p - 1, rng.randrange(p)]), rng.choice([1, p - 1, rng.randrange(p)])
            e = (c1 * x * y + c2 + x) ** 2 % p
            rows_i.append([(e + 1) % p if lane % 3 == 1 else e])   # every third lane corrupted
            rows_w.append([x, y])
        return rows_i, rows_w
    return rel, lanes


@pytest.mark.gpu
@pytest.mark.parametrize('p', ROW_MODULI)
def test_rows_from_the_tape_checked_on_the_gpu(p):
    """rows from the tape, the replay's wire table, the row kernel: the same verdict as the replay on every lane of two
    or more lane blocks, and every failing row is an assert row"""
    batch = 70
    for which in ('checked', 'random'):
        if which == 'checked':
            rel, lanes = _checked_relation(p)
            n_inst, n_wit = 1, 2
            rows_i, rows_w = lanes(batch, p.bit_length())
        else:
            g, rel, _ = _gen(p, 900 + p.bit_length())
            n_inst, n_wit = g.n_inst, g.n_wit
            rows_i, rows_w = g.lane_inputs(batch, 77)
        ev = zk.Evaluator()
        ev.declare_inputs(n_inst, n_wit)
        ev.ingest_message(rel)
        ev.finalize(retain_all=True)
        ev.r1cs_from_tape()
        inst, wit = batch_arrays(rows_i, rows_w, ev.elem_bytes)
        ev.set_inputs(inst, wit, batch)
        ev.replay()
        ev.synchronize()
        ev.r1cs_check()
        ff, counts = ev.r1cs_results(batch)
        assert counts == ev.counts(), (p, which)
        first, _ = ev.lane_results(batch)
        assert [int(x) == zk.NO_FAIL for x in ff] == [int(x) == zk.NO_FAIL for x in first], (p, which)
        rows, _ = ev.r1cs_export()
        for x in ff:
            if int(x) != zk.NO_FAIL:
                assert rows[int(x)][2] == [(0, 0)], (p, which, int(x))
        if which == 'checked':
            assert counts == (batch - batch // 3, batch // 3), p


def _csr_with_false_row(wl, p, coef_kind, seed):
    """wl's CSR with coefficients of the field's whole width (random kind: the generator's stop at 2^256) and one false
    row appended: (z_0) * (one) = (z_0 + 1)"""
    row_ptr, tv, tc, cb = wl.csr()
    if coef_kind == 'random' and p.bit_length() > 256:
        rnd = random.Random(seed)
        cb = cb.copy()
        for i in range(len(cb) - 1):
            cb[i] = np.frombuffer(_le(rnd.randrange(p), wl.width), dtype=np.uint8)
    one = len(cb) - 1
    z0 = wl.n_base + 1
    t0 = int(row_ptr[-1])
    row_ptr = np.concatenate([row_ptr, np.array([t0 + 1, t0 + 2, t0 + 4], dtype=np.uint32)])
    tv = np.concatenate([tv, np.array([z0, NO_VAR, z0, NO_VAR], dtype=np.uint64)])
    tc = np.concatenate([tc, np.array([one] * 4, dtype=np.uint32)])
    return row_ptr, tv, tc, cb


def _csr_run(p, coef_kind, batch, devices=None, classes='1'):
    """assign the rows level by level, reload E := z_last, check; returns (ev, wl, csr, witnesses, first_fail, counts)"""
    wl = workloads.R1csSynthetic(M=300, n_base=24, n_coefs=50, seed=5, p=p, coef_kind=coef_kind)
    ev = zk.Evaluator()
    ev.set_option('r1cs_coef_classes', classes)
    if devices:
        ev.set_option('devices', devices)
    ev.declare_inputs(0, wl.n_witness)
    ev.ingest_message(wl.base_relation())
    ev.finalize(retain_all=True)
    row_ptr, tv, tc, cb = _csr_with_false_row(wl, p, coef_kind, 5)
    ev.r1cs_load_csr(row_ptr, tv, tc, cb, wl.width, wl.M)
    w = wl.witnesses(batch)
    ev.set_inputs(None, w.tobytes(), batch)
    ev.replay()
    lo = 0
    for hi in wl.level_bounds:
        ev.r1cs_assign(lo, int(hi) - lo)
        lo = int(hi)
    assert lo == wl.M
    zl = ev.r1cs_get_var(wl.last_z, batch)
    for lane in range(batch):
        w[lane, wl.n_base] = np.frombuffer(_le(zl[lane], wl.width), dtype=np.uint8)
    ev.set_inputs(None, w.tobytes(), batch)
    ev.replay()
    ev.r1cs_check()
    ff, counts = ev.r1cs_results(batch)
    return ev, wl, (row_ptr, tv, tc, cb), w, ff, counts


CSR_MODULI = [2 ** 64, 2 ** 64 - 2, 2 ** 160, 2 ** 224 - 2, 2 ** 256 - 2, 2 ** 521 - 1, ODD1024, 2 ** 4096 - 1]


@pytest.mark.gpu
@pytest.mark.parametrize('coef_kind', ['random', 'small'])
@pytest.mark.parametrize('p', CSR_MODULI)
def test_csr_rows_with_coefficients_on_the_gpu(p, coef_kind):
    """a caller's CSR (3 + 3 term products): witness generation by the row kernel level by level, sampled values against
    Python integers, then the check; the appended false row fails on every lane.  K = 3, 2, 6, 7, 8 words and the wide
    classes."""
    batch = 67
    ev, wl, (row_ptr, tv, tc, cb), w, ff, counts = _csr_run(p, coef_kind, batch)
    coefs = [int.from_bytes(cb[i].tobytes(), 'little') for i in range(len(cb))]
    for lane in (0, 33, batch - 1):
        val = {k: int.from_bytes(w[lane, k].tobytes(), 'little') for k in range(wl.n_witness)}
        for r in range(wl.M):
            terms = [(int(tv[7 * r + k]), coefs[int(tc[7 * r + k])]) for k in range(6)]
            a = sum(c * val[v] for v, c in terms[:3]) % p
            b = sum(c * val[v] for v, c in terms[3:]) % p
            val[wl.n_base + 1 + r] = a * b % p
        for var in (wl.n_base + 1, wl.n_base + 1 + wl.M // 2, wl.last_z):
            assert ev.r1cs_get_var(var, batch)[lane] == val[var], (p, lane, var)
    assert counts == (0, batch)
    assert all(int(x) == wl.M + 1 for x in ff)
    cc = ev.r1cs_class_counts()
    assert cc['unit'] == 0 and cc['small'] == 0


def _bound_system(p, n_base, n_terms=255):
    """Caller ids: witness k is k, the extra variable z is n_base.  Coefficient 0 is 1, coefficient 1 is p - 1.
    row 0: (255 x (p - 1) w0) * (255 x (p - 1) w1) = (z), assigned
    row 1: (255 x (p - 1) w0) * (one) = (255 x (p - 1) w1): true, since w0 = w1
    row 2: (255 x (p - 1) w0) * (one) = (254 x (p - 1) w1): false unless (p - 1) w1 = 0 mod p"""
    width = _width(p)
    rows = [([(0, 1)] * n_terms, [(1, 1)] * n_terms, [(n_base, 0)]),
            ([(0, 1)] * n_terms, [(NO_VAR, 0)], [(1, 1)] * n_terms),
            ([(0, 1)] * n_terms, [(NO_VAR, 0)], [(1, 1)] * (n_terms - 1))]
    tv, tc, row_ptr = [], [], [0]
    for row in rows:
        for comb in row:
            tv += [v for v, _ in comb]
            tc += [c for _, c in comb]
            row_ptr.append(len(tv))
    return (np.array(row_ptr, dtype=np.uint32), np.array(tv, dtype=np.uint64), np.array(tc, dtype=np.uint32),
            np.frombuffer(_le(1, width) + _le(p - 1, width), dtype=np.uint8).reshape(2, width))


@pytest.mark.gpu
@pytest.mark.parametrize('p', BOUND_MODULI)
def test_combination_bounds_on_the_gpu(p):
    """255-term combinations of p - 1 (coefficients and values) through assign and check on the card"""
    n_base, batch = 4, 70
    width = _width(p)
    row_ptr, tv, tc, cb = _bound_system(p, n_base)
    ev = zk.Evaluator()
    ev.declare_inputs(0, n_base)
    ev.ingest_message(sw.write_relation(sw.int_to_le(p), 'arithmetic', 'simple', [], [('witness', k) for k in range(n_base)]))
    ev.finalize(retain_all=True)
    ev.r1cs_load_csr(row_ptr, tv, tc, cb, width, 1)
    rnd = random.Random(p.bit_length())
    vals = [[p - 1] * n_base if lane % 4 else [rnd.randrange(p)] * n_base for lane in range(batch)]
    ev.set_inputs(None, b''.join(_le(v, width) for row in vals for v in row), batch)
    ev.replay()
    ev.r1cs_assign(0, 1)
    z = ev.r1cs_get_var(n_base, batch)
    for lane in range(batch):
        s = 255 * (p - 1) * vals[lane][0] % p
        assert z[lane] == s * s % p, (p, lane)
    ev.r1cs_check()
    ff, counts = ev.r1cs_results(batch)
    for lane in range(batch):
        s = 255 * (p - 1) * vals[lane][0] % p
        row2_holds = (p - 1) * vals[lane][0] % p == 0
        assert int(ff[lane]) == (zk.NO_FAIL if row2_holds else 2), (p, lane)


@pytest.mark.gpu
@pytest.mark.parametrize('p', [2 ** 521 - 1, ODD1024, 2 ** 64 - 2, 6 * 2 ** 100 + 6, 2 ** 256 - 2, 2 ** 64, 2 ** 4095, 2 ** 4096 - 1])
def test_quotient_wires_on_the_gpu(p):
    """the quotient wire of every add / mul / add_constant / mul_constant call, against (x op y) // p from the oracle's
    values, lane by lane: odd wide moduli, even ones (2^s * m) and powers of two"""
    lanes = 70
    rel, make_lanes = _checked_relation(p)
    rows_i, rows_w = make_lanes(lanes, 3)
    ev = zk.Evaluator()
    ev.declare_inputs(1, 2)
    ev.ingest_message(rel)
    ev.finalize(retain_all=True)
    ev.r1cs_from_tape(use_correction=True)
    inst, wit = batch_arrays(rows_i, rows_w, ev.elem_bytes)
    ev.set_inputs(inst, wit, lanes)
    ev.replay()
    ev.synchronize()
    kinds, a, b = ev.tape()
    consts = [int.from_bytes(c, 'little') for c in ev.constants()]
    calls = [i for i, k in enumerate(kinds) if int(k) in (1, 2, 3, 4)]
    assert sorted(set(int(kinds[i]) for i in calls)) == [1, 2, 3, 4]
    got = ev.r1cs_correction_values(calls, lanes)
    value_index = {i: t for t, i in enumerate(j for j, k in enumerate(kinds) if int(k) != 9)}
    mod_le = sw.int_to_le(p)
    for lane in range(lanes):
        vals = oracle_lane(mod_le, rows_i[lane], rows_w[lane], [rel], _width(p)).trace_values()
        for n, i in enumerate(calls):
            x = vals[value_index[int(a[i])]]
            k = int(kinds[i])
            y = vals[value_index[int(b[i])]] if k in (1, 2) else consts[int(b[i])]
            full = x + y if k in (1, 3) else x * y
            assert full % p == vals[value_index[i]]
            assert got[lane][n] == full // p, (p, lane, i, k)


@pytest.mark.gpu
@pytest.mark.parametrize('p', [2 ** 64 - 2, 2 ** 64, 2 ** 521 - 1])
def test_rows_and_their_ir_expansion_agree_per_lane(p):
    """One constraint system over a canonical-residue field, two device paths: the row kernel over the CSR and the replay
    of its FromR1CSConverter expansion.  Every lane gets the same verdict, and the first failing row is the first failing
    assert."""
    from zkinterface_ir_amd.builder import MemorySink
    from zkinterface_ir_amd.from_r1cs import FromR1CSConverter
    rng = random.Random(1234)
    n_base, M, batch = 12, 120, 70
    width = _width(p)
    rows = []   # ids: 0 = one, 1..n_base base, n_base+1+i = z_i
    for i in range(M):
        hi = n_base + 1 + i
        lc = lambda k: [(rng.randrange(hi), rng.randrange(p)) for _ in range(k)]
        rows.append((lc(rng.randrange(1, 4)), lc(rng.randrange(0, 4)), [(hi, 1)]))
    vals = [[0] * (n_base + 1 + M) for _ in range(batch)]
    bad_row = {}
    for lane in range(batch):
        vals[lane][0] = 1
        for k in range(1, n_base + 1):
            vals[lane][k] = rng.randrange(p)
        wrong = rng.randrange(M) if lane % 5 == 2 else None
        for i, (A, B, _c) in enumerate(rows):
            z = sum(c * vals[lane][v] for v, c in A) % p * (sum(c * vals[lane][v] for v, c in B) % p) % p
            if wrong == i:
                z = (z + 1) % p
                bad_row[lane] = i
            vals[lane][n_base + 1 + i] = z
    n_wit = n_base + M
    wit = b''.join(_le(vals[lane][k], width) for lane in range(batch) for k in range(1, n_wit + 1))

    cb = [_le(1, width)]
    tv, tc, row_ptr = [], [], [0]
    for A, B, C in rows:
        for comb in (A, B, C):
            for var, coef in comb:
                tv.append(NO_VAR if var == 0 else var - 1)
                cb.append(_le(coef, width))
                tc.append(len(cb) - 1)
            row_ptr.append(len(tv))
    ev = zk.Evaluator()
    ev.declare_inputs(0, n_wit)
    ev.ingest_message(sw.write_relation(sw.int_to_le(p), 'arithmetic', 'simple', [], [('witness', k) for k in range(n_wit)]))
    ev.finalize(retain_all=True)
    ev.r1cs_load_csr(np.array(row_ptr, dtype=np.uint32), np.array(tv, dtype=np.uint64), np.array(tc, dtype=np.uint32),
                     np.frombuffer(b''.join(cb), dtype=np.uint8).reshape(len(cb), width), width, 0)
    ev.set_inputs(None, wit, batch)
    ev.replay()
    ev.r1cs_check()
    ff_rows, counts_rows = ev.r1cs_results(batch)

    conv = FromR1CSConverter(MemorySink(), p - 1, [(0, _le(1, width))], list(range(1, n_wit + 1)))
    conv.ingest_constraints([tuple([(var, _le(c, width)) for var, c in comb] for comb in row) for row in rows])
    rel = conv.finish().buffers()[2]
    ev2 = zk.Evaluator()
    ev2.declare_inputs(0, n_wit)
    ev2.ingest_message(rel)
    ev2.finalize()
    assert ev2.field_representation(0) == 2
    ev2.set_inputs(None, wit, batch)
    ev2.replay()
    ev2.synchronize()
    ff_gates, _ = ev2.lane_results(batch)
    assert ev2.counts() == counts_rows == (batch - len(bad_row), len(bad_row))
    for lane in range(batch):
        want = bad_row.get(lane, zk.NO_FAIL)
        assert int(ff_rows[lane]) == want and int(ff_gates[lane]) == want, lane


@pytest.mark.gpu
@pytest.mark.parametrize('p', [2 ** 64 - 2, 2 ** 521 - 1])
def test_two_engines_give_the_single_engine_results(p):
    """option devices = "0,0": two engines share the lanes; every value and verdict equals the single engine's"""
    batch = 130
    ev1, wl, _, _, ff1, counts1 = _csr_run(p, 'random', batch)
    ev2, _, _, _, ff2, counts2 = _csr_run(p, 'random', batch, devices='0,0')
    assert counts1 == counts2 == (0, batch)
    assert [int(x) for x in ff1] == [int(x) for x in ff2]
    assert ev1.r1cs_get_var(wl.last_z, batch) == ev2.r1cs_get_var(wl.last_z, batch)
