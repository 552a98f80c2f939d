"""The Montgomery kernels (zkinterface-ir_amd/csrc/device/fp_mont.hpp) at every width they are compiled for -- 2, 4, ..., 16
words of 32 bits -- times the moduli that sit on their reduction bounds (mont_cases.py), in every kernel family that calls
them: replay_kernel, replay_fused_kernel, replay_strand_kernel, r1cs_row_kernel, r1cs_correction_kernel.  Operands are
chosen in the Montgomery domain (0, 1, p - 1, words of 0xFFFFFFFF, sums of exactly p and exactly R ...), so that the carry
chains, the conditional subtractions and the multi-round reduction of fp_dot meet their edges on purpose instead of with
probability 2^-32.  The reference is Python integers; every comparison is exact.

The CPU tier sends the same relations through recording, scheduling and program_sim (the host half: constant pool in
Montgomery form, words per constant, slot reuse), and checks the per-field constants the kernels are launched with."""
import random

import numpy as np
import pytest

import mont_cases as mc
import program_sim
import zkinterface_ir_amd as zk
from zkinterface_ir_amd import sieve_writer as sw

CELLS = [pytest.param(n, c, id='w%d-%s' % (n, c)) for n in mc.WIDTHS for c in mc.CLASSES]
cells = pytest.mark.parametrize('width,cls', CELLS)


def _le(v, nbytes):
    return int(v).to_bytes(nbytes, 'little')


def _mod_le(p):
    return _le(p, max(4, (p.bit_length() + 7) // 8))


def _rows_bytes(rows, nbytes):
    return b''.join(_le(v, nbytes) for r in rows for v in r)


def _session(p, gates, n_inst, n_wit, retain_all=False, options=(), functions=(), gateset='arithmetic', features='simple'):
    ev = zk.Evaluator()
    for k, v in options:
        ev.set_option(k, v)
    ev.declare_inputs(n_inst, n_wit)
    ev.ingest_message(sw.write_relation(_mod_le(p), gateset, features, list(functions), gates))
    assert ev.host_violations() == []
    ev.finalize(retain_all=retain_all)
    assert ev.field_representation() == 1           # Montgomery form
    return ev


def _run(ev, inst_rows, wit_rows):
    w = ev.elem_bytes
    ev.set_inputs(_rows_bytes(inst_rows, w) if inst_rows and inst_rows[0] else None, _rows_bytes(wit_rows, w), len(wit_rows))
    ev.replay()
    ev.synchronize()


def _kinds(ops):
    k = ops[:, 1]
    return k & 0xFF, (k >> 8) & 3, (k >> 10) & 3, (k >> 12) & 3


# ------------------------------------------------------------------------------------------------ gate kernels, unfused
def gate_constants(p, width):
    """constants of the addc / mulc gates, as canonical values: chosen by the word pattern the kernel holds for them"""
    R = 1 << (32 * width)
    ms = [p - 1, (p + 1) // 2, mc.all_ones_below(p), R % p]
    return [mc.from_mont(m, p, width) for m in ms] + [p - 1]


def gate_relation(p, width):
    """one operand pair per lane: add, mul, squares, and addc / mulc by each constant"""
    nb = 4 * width
    gates = [('witness', 0), ('witness', 1), ('add', 2, 0, 1), ('mul', 3, 0, 1), ('mul', 4, 0, 0), ('add', 5, 1, 1), ('mul', 6, 1, 1)]
    w = 7
    for c in gate_constants(p, width):
        for src in (0, 1):
            gates += [('addc', w, src, _le(c, nb)), ('mulc', w + 1, src, _le(c, nb))]
            w += 2
    gates += [('mul', w, 3, 2), ('add', w + 1, w, 3)]         # (operands that are results, not inputs)
    return gates


def gate_lanes(p, width, n_random=4):
    """canonical witness pairs: x = m / R for the Montgomery-domain pairs of mont_cases, then canonical edges; the last
    64-lane block is ragged"""
    pairs = [(mc.from_mont(a, p, width), mc.from_mont(b, p, width)) for a, b in mc.operand_pairs(p, width, n_random)]
    pairs += [(p - 1, p - 1), (p - 1, 1), (1, p - 1), (0, p - 1), (p - 1, 0), ((p - 1) // 2, (p + 1) // 2), (p - 2, 2)]
    while len(pairs) % 64 in (0, 63):
        pairs.append((p - 1 - len(pairs) % p, (3 * len(pairs)) % p))
    return pairs


@pytest.mark.gpu
@cells
def test_unfused_gate_kernel_every_wire(width, cls):
    """replay_kernel (the retain_all schedule): every wire of every lane against Python integers"""
    p = mc.modulus(width, cls)
    gates = gate_relation(p, width)
    lanes = gate_lanes(p, width)
    ev = _session(p, gates, 0, 2, retain_all=True)
    assert ev.elem_bytes == 4 * width
    ops, launches, _, _ = ev.schedule_dump()
    kind, ea, eb, second = _kinds(ops)
    # the unfused program: no operand expression, no pair entry, no strand -- every launch is replay_kernel
    assert not ea.any() and not eb.any() and not second.any()
    assert all(ev.strand_levels(k) is None for k in range(len(launches)))
    assert {1, 2, 3, 4} <= set(int(k) for k in kind)
    _run(ev, None, lanes)
    got = ev.dump_trace_values(len(lanes))
    for lane, (a, b) in enumerate(lanes):
        _, trace, _ = mc.evaluate_gates(gates, p, [], [a, b])
        assert got[lane] == trace, (lane, hex(a), hex(b), [i for i in range(len(trace)) if got[lane][i] != trace[i]])


@cells
def test_unfused_gate_relation_on_the_host(width, cls):
    p = mc.modulus(width, cls)
    gates = gate_relation(p, width)
    lanes = gate_lanes(p, width, n_random=1)
    ev = _session(p, gates, 0, 2, retain_all=True)
    ops, launches, consts, slot_of = ev.schedule_dump()
    info = ev.schedule_info()
    assert info['words_per_const'] == width
    kinds, _, _ = ev.tape()
    for lane in list(range(0, len(lanes), 7)) + [len(lanes) - 7]:
        a, b = lanes[lane]
        slots, ff, noncanon = program_sim.simulate(ops, launches, consts, width, info['slots'], p, [], [a, b], shuffle_seed=lane)
        _, trace, _ = mc.evaluate_gates(gates, p, [], [a, b])
        vals = [program_sim.from_device_form(slots[slot_of[i]], p, width) for i in range(len(kinds)) if kinds[i] != 9]
        assert not noncanon and ff is None and vals == trace, lane


# ------------------------------------------------------------------------------------ gate kernels, production schedule
LAYER_W, LAYER_D, LAYER_OUT = 32, 5, 8


def layered_relation(p, width):
    """A relation the scheduler fuses: LAYER_W witness inputs; layer 1 adds and multiplies the input pairs (2i, 2i + 1);
    then LAYER_D layers of adds / products of two wires of the layer before (single-reader producers that fold into their
    reader's operand expression, two-reader producers, pairs of gates that share an operand), each layer freed once read;
    the first LAYER_OUT wires of the last layer are compared with instance values and stay alive for Evaluator::get.
    Returns (gates, ids of the output wires)."""
    rng = random.Random('%d/layered/%d' % (mc.SEED, width))
    W = LAYER_W
    nb = 4 * width
    gates = [('witness', k) for k in range(W)]
    for i in range(W // 2):
        gates += [('add', W + 2 * i, 2 * i, 2 * i + 1), ('mul', W + 2 * i + 1, 2 * i, 2 * i + 1)]
    gates.append(('free', 0, W - 1))
    for l in range(2, LAYER_D + 2):
        prev, base = (l - 1) * W, l * W
        for j in range(W):
            a, b = prev + rng.randrange(W), prev + rng.randrange(W)
            if j % 8 == 7:
                gates.append((('addc', 'mulc')[(j // 8) % 2], base + j, a, _le(gate_constants(p, width)[(j // 8 + l) % 5], nb)))
            else:
                gates.append((('add', 'mul')[rng.randrange(2)], base + j, a, b))
        gates.append(('free', prev, prev + W - 1))
    last = (LAYER_D + 1) * W
    e = last + W
    for t in range(LAYER_OUT):
        gates += [('instance', e + 3 * t), ('mulc', e + 3 * t + 1, e + 3 * t, _le(p - 1, nb)), ('add', e + 3 * t + 2, last + t, e + 3 * t + 1),
                  ('assert_zero', e + 3 * t + 2)]
    gates.append(('free', e, e + 3 * LAYER_OUT - 1))
    return gates, [last + t for t in range(LAYER_OUT)]


def layered_lanes(p, width, n_lanes, n_random=4):
    """lane L takes LAYER_W / 2 consecutive operand pairs (as canonical values) starting at pair 16 L: every pair meets the
    add and the product of layer 1 in some lane"""
    pairs = [(mc.from_mont(a, p, width), mc.from_mont(b, p, width)) for a, b in mc.operand_pairs(p, width, n_random)]
    return [[v for i in range(LAYER_W // 2) for v in pairs[(lane * (LAYER_W // 2) + i) % len(pairs)]] for lane in range(n_lanes)]


def layered_expectations(p, gates, outs, wit_rows, corrupt_every=5):
    """(instance rows, output values per lane, first failing assert per lane or None): the expected outputs, one of them
    off by one on every corrupt_every-th lane"""
    inst_rows, values, fails = [], [], []
    for lane, wit in enumerate(wit_rows):
        wires, _, _ = mc.evaluate_gates(gates, p, [0] * LAYER_OUT, wit)
        exp = [wires[o] for o in outs]
        values.append(list(exp))
        bad = lane % LAYER_OUT if lane % corrupt_every == 0 else None
        if bad is not None:
            exp[bad] = (exp[bad] + 1) % p
        inst_rows.append(exp)
        _, _, ff = mc.evaluate_gates(gates, p, exp, wit)
        assert ff == bad
        fails.append(ff)
    return inst_rows, values, fails


def _assert_fused_program(ev):
    """the launches of replay_fused_kernel (the ones that are not strands) hold operand expressions and pair entries"""
    ops, launches, _, _ = ev.schedule_dump()
    fused = np.zeros(len(ops), dtype=bool)
    for k, (first, count, _, sequential) in enumerate(launches):
        if not sequential:
            assert ev.strand_levels(k) is None
            fused[int(first):int(first) + int(count)] = True
    kind, ea, eb, second = (x[fused] for x in _kinds(ops))
    assert int((ea != 0).sum()) + int((eb != 0).sum()) >= 8, 'no operand expressions: the relation was not fused'
    assert int((second != 0).sum()) >= 2, 'no pair entries'
    assert {1, 2} <= set(int(k) for k in kind[(ea != 0) | (eb != 0)])        # add and mul readers of an expression
    assert {1, 2} <= set(int(e) for e in np.concatenate([ea, eb]) if e)     # add and mul expressions


# strand_width 1: only the levels of one or two entries go to a sequential launch, every other level is a launch of
# replay_fused_kernel
FUSED_ONLY = (('strand_width', '1'),)


@pytest.mark.gpu
@cells
def test_fused_gate_kernel_outputs_and_verdicts(width, cls):
    """replay_fused_kernel (the production schedule): surviving wires through Evaluator::get and assert_zero verdicts"""
    p = mc.modulus(width, cls)
    gates, outs = layered_relation(p, width)
    n_lanes = 70
    wit = layered_lanes(p, width, n_lanes)
    inst, values, fails = layered_expectations(p, gates, outs, wit)
    ev = _session(p, gates, LAYER_OUT, LAYER_W, options=FUSED_ONLY)
    _assert_fused_program(ev)
    _run(ev, inst, wit)
    first, flags = ev.lane_results(n_lanes)
    assert not flags.any()
    assert [None if int(x) == zk.NO_FAIL else int(x) for x in first] == fails
    n_bad = sum(f is not None for f in fails)
    assert ev.counts() == (n_lanes - n_bad, n_bad) and 0 < n_bad < n_lanes
    for t, o in enumerate(outs):
        got = ev.get(o, n_lanes)
        assert got == [values[lane][t] for lane in range(n_lanes)], (t, [l for l in range(n_lanes) if got[l] != values[l][t]])


@cells
def test_fused_gate_relation_on_the_host(width, cls):
    p = mc.modulus(width, cls)
    gates, outs = layered_relation(p, width)
    wit = layered_lanes(p, width, 6, n_random=1)
    inst, _, fails = layered_expectations(p, gates, outs, wit)
    ev = _session(p, gates, LAYER_OUT, LAYER_W, options=FUSED_ONLY)
    _assert_fused_program(ev)
    ops, launches, consts, _ = ev.schedule_dump()
    info = ev.schedule_info()
    assert info['words_per_const'] == width
    for lane in range(len(wit)):
        _, ff, noncanon = program_sim.simulate(ops, launches, consts, width, info['slots'], p, inst[lane], wit[lane], shuffle_seed=lane)
        assert not noncanon and ff == fails[lane], lane
        # every output on its own: the verdict moves to the assert whose expected value is wrong
        for t in range(LAYER_OUT):
            row = list(inst[lane])
            row[t] = (row[t] + 2) % p
            _, ff, _ = program_sim.simulate(ops, launches, consts, width, info['slots'], p, row, wit[lane])
            assert ff == (t if fails[lane] is None else min(t, fails[lane])), (lane, t)


# ---------------------------------------------------------------------------------------------------------------- strands
CHAIN_N = 6


def chain_relation(p):
    """The reference's example shape (For over a named function with a nested call and a Switch) with every iteration
    reading the previous one's result -- workloads.StructuredArith(chained=True) -- except that every link of the chain is
    compared with an instance value and stays alive:  step(o; a, b, c):  t = a * b;  switch c { 0: o = t + a;  1: o = t * b }.
    Witness b_i = i, c_i = N + i, acc_0 = 2N; acc_{i+1} = 2N + 1 + i; expected e_i (instance)."""
    N = CHAIN_N
    neg_one = sw.int_to_le(p - 1)
    functions = [
        ('mm::mul', 1, 2, 0, 0, [('mul', 0, 1, 2)]),
        ('mm::step', 1, 3, 0, 0, [
            ('call', 'mm::mul', [4], [1, 2]),
            ('switch', 3, [0], [bytes([0]), bytes([1])], [
                ('anon', [4, 1], 0, 0, [('add', 0, 1, 2)]),
                ('anon', [4, 2], 0, 0, [('mul', 0, 1, 2)]),
            ]),
            ('free', 4, None),
        ]),
    ]
    gates = [('witness', k) for k in range(2 * N + 1)]
    gates.append(('for', 'i', 0, N - 1, [(2 * N + 1, 3 * N)],
                  ('call', 'mm::step', [('add', ('name', 'i'), ('const', 2 * N + 1))],
                   [('add', ('name', 'i'), ('const', 2 * N)), ('name', 'i'), ('add', ('name', 'i'), ('const', N))])))
    e = 3 * N + 1
    for i in range(N):
        gates += [('instance', e + 3 * i), ('mulc', e + 3 * i + 1, e + 3 * i, neg_one), ('add', e + 3 * i + 2, 2 * N + 1 + i, e + 3 * i + 1),
                  ('assert_zero', e + 3 * i + 2)]
    gates.append(('free', e, e + 3 * N - 1))
    return functions, gates


def chain_reference(p, wit):
    N = CHAIN_N
    acc, out = wit[2 * N], []
    for i in range(N):
        t = mc.ref_mul(acc, wit[i], p)
        acc = mc.ref_mul(t, wit[i], p) if wit[N + i] else mc.ref_add(t, acc, p)
        out.append(acc)
    return out


def chain_lanes(p, width, n_lanes, n_random=4):
    """b_i and acc_0 from the operand set (canonical values of the Montgomery-domain edges), c_i alternating by lane; every
    fifth lane claims one wrong link"""
    N = CHAIN_N
    vals = [mc.from_mont(m, p, width) for m in mc.edge_mont_values(p, width, n_random)]
    wit, inst, fails = [], [], []
    for lane in range(n_lanes):
        w = [vals[(lane * (N + 1) + i) % len(vals)] for i in range(N)] + [(lane >> (i % 3) ^ i) & 1 for i in range(N)] + \
            [vals[(lane * (N + 1) + N) % len(vals)]]
        exp = chain_reference(p, w)
        bad = lane % N if lane % 5 == 0 else None
        if bad is not None:
            exp[bad] = (exp[bad] + 1) % p
        wit.append(w)
        inst.append(exp)
        fails.append(bad)
    return wit, inst, fails


def _chain_session(p):
    functions, gates = chain_relation(p)
    return _session(p, gates, CHAIN_N, 2 * CHAIN_N + 1, functions=functions, gateset='@add,@mul,@mulc,',
                    features='@for,@switch,@function,')


def _assert_strand_program(ev):
    """a sequential launch exists, it holds products and sums, and the static rule that makes the sequential simulator's
    result the kernel's holds for it (test_strands.py)"""
    ops, launches, _, _ = ev.schedule_dump()
    strands = [(k, ev.strand_levels(k)) for k in range(len(launches)) if ev.strand_levels(k) is not None]
    assert strands, 'no sequential launch: replay_strand_kernel did not run'
    kinds_in_strands = set()
    for k, (level_ptr, lds_slots) in strands:
        first, count = int(launches[k][0]), int(launches[k][1])
        assert launches[k][3]
        assert int(level_ptr[0]) == 0 and int(level_ptr[-1]) == count
        assert program_sim.strand_hazards(ops, first, level_ptr) == []
        kinds_in_strands |= set(int(x) & 0xFF for x in ops[first:first + count, 1])
    assert {1, 2} <= kinds_in_strands
    return ops, launches


@pytest.mark.gpu
@cells
def test_strand_kernel_chain_links_and_verdicts(width, cls):
    """replay_strand_kernel: every link of a dependency chain (Evaluator::get) and the verdicts, over the prime nearest the
    class's modulus (the Switch weights are a^(p - 1))"""
    p = mc.prime_modulus(width, cls)
    n_lanes = 70
    wit, inst, fails = chain_lanes(p, width, n_lanes)
    ev = _chain_session(p)
    _assert_strand_program(ev)
    _run(ev, inst, wit)
    first, flags = ev.lane_results(n_lanes)
    assert not flags.any()
    assert [None if int(x) == zk.NO_FAIL else int(x) for x in first] == fails
    for i in range(CHAIN_N):
        got = ev.get(2 * CHAIN_N + 1 + i, n_lanes)
        want = [chain_reference(p, w)[i] for w in wit]
        assert got == want, (i, [l for l in range(n_lanes) if got[l] != want[l]])


@cells
def test_strand_relation_on_the_host(width, cls):
    p = mc.prime_modulus(width, cls)
    assert mc.is_probable_prime(p)
    wit, inst, fails = chain_lanes(p, width, 6, n_random=1)
    ev = _chain_session(p)
    ops, launches = _assert_strand_program(ev)
    _, _, consts, _ = ev.schedule_dump()
    info = ev.schedule_info()
    assert info['words_per_const'] == width
    for lane in range(len(wit)):
        _, ff, noncanon = program_sim.simulate(ops, launches, consts, width, info['slots'], p, inst[lane], wit[lane])
        assert not noncanon and ff == fails[lane], lane
        for t in range(CHAIN_N):         # each link on its own
            row = list(inst[lane])
            row[t] = (row[t] + 2) % p
            _, ff, _ = program_sim.simulate(ops, launches, consts, width, info['slots'], p, row, wit[lane])
            assert ff == (t if fails[lane] is None else min(t, fails[lane])), (lane, t)


# ------------------------------------------------------------------------------------------------------------- R1CS rows
R1CS_BASE = 16
ONE_VAR = 2 ** 64 - 1
TERM_COUNTS = (1, 2, 3, 4, 6, 7)          # chunks of 3, 2 and 1 products; one chunk of 3 is the lazy case


def r1cs_system(p, width):
    """A constraint system over R1CS_BASE witness variables.  Returns (pool of coefficients, rows to assign in two levels,
    check-only rows); a row is (A, B, C), a combination a list of (variable, pool index), ONE_VAR the constant one.
    Pool: index 0 is the coefficient 1; 1 has the Montgomery form p - 1 (the largest word pattern a coefficient can
    have); the rest are the other edges and random values -- all of class `full` unless p is tiny."""
    R = 1 << (32 * width)
    ms = [p - 1, (p + 1) // 2, mc.all_ones_below(p), 2, 1, p - 2] + mc.edge_mont_values(p, width, 6, seed=1)[-6:]
    pool = [1] + [c for c in dict.fromkeys(mc.from_mont(m, p, width) for m in ms) if c not in (0, 1)]
    assert mc.to_mont(pool[1], p, width) == p - 1
    rng = random.Random('%d/r1cs/%d' % (mc.SEED, width))
    n_full = len(pool) - 1
    z = [R1CS_BASE]

    def comb(n, coef=None, one_at=None):
        return [(ONE_VAR if k == one_at else rng.randrange(R1CS_BASE), coef if coef is not None else 1 + rng.randrange(n_full))
                for k in range(n)]

    def out():
        z[0] += 1
        return [(z[0] - 1, 0)]
    level1 = [(comb(na), comb(nb), out()) for na in TERM_COUNTS for nb in TERM_COUNTS]
    # every coefficient with the Montgomery form p - 1 (lane 0 holds p - 1 in every variable: the largest sums)
    level1 += [(comb(na, coef=1), comb(nb, coef=1), out()) for na, nb in ((3, 3), (7, 7), (4, 6), (2, 1), (6, 3), (3, 2), (1, 3))]
    # B = 1 (kR1csBIsOne), and the constant one as a term of A and of B
    level1 += [(comb(na), [(ONE_VAR, 0)], out()) for na in TERM_COUNTS]
    level1 += [(comb(3, one_at=1), comb(3, one_at=2), out()), (comb(4, one_at=3), comb(2, one_at=0), out()),
               (comb(3, coef=1, one_at=0), comb(3, coef=1, one_at=0), out())]
    n1 = z[0] - R1CS_BASE
    # second level: combinations of the assigned variables
    def zcomb(n, coef=None):
        return [(R1CS_BASE + rng.randrange(n1), coef if coef is not None else 1 + rng.randrange(n_full)) for _ in range(n)]
    level2 = [(zcomb(3), zcomb(3), out()), (zcomb(3, coef=1), zcomb(3, coef=1), out()), (zcomb(7), zcomb(2), out()), (zcomb(1), zcomb(4), out())]
    # check only: X * 1 = X puts combinations of every size on the C side
    checks = []
    for n in TERM_COUNTS:
        x = comb(n) if n != 3 else comb(3, coef=1)
        checks.append((x, [(ONE_VAR, 0)], list(x)))
    return pool, [level1, level2], checks


def r1cs_values(p, width, n_lanes):
    """lane 0: every variable holds the word pattern p - 1; the others walk the operand set"""
    vals = [mc.from_mont(m, p, width) for m in mc.edge_mont_values(p, width, 4)]
    rows = [[mc.from_mont(p - 1, p, width)] * R1CS_BASE]
    for lane in range(1, n_lanes):
        rows.append([vals[(lane * 5 + 3 * k) % len(vals)] for k in range(R1CS_BASE)])
    return rows


def _terms(comb):
    return [(None if v == ONE_VAR else v, c) for v, c in comb]


def r1cs_reference(p, pool, levels, checks, base):
    """(values of all variables after assignment, function: values -> first failing row or None)"""
    vals = list(base)
    rows = [r for lvl in levels for r in lvl]
    for a, b, c in rows:
        assert c[0][0] == len(vals)
        vals.append(mc.ref_row([(v, pool[k]) for v, k in _terms(a)], [(v, pool[k]) for v, k in _terms(b)], vals, p))

    def first_fail(v):
        for r, (a, b, c) in enumerate(rows + checks):
            if mc.ref_row([(x, pool[k]) for x, k in _terms(a)], [(x, pool[k]) for x, k in _terms(b)], v, p) != \
                    mc.ref_lincomb([(x, pool[k]) for x, k in _terms(c)], v, p):
                return r
        return None
    return vals, first_fail


@pytest.mark.gpu
@pytest.mark.parametrize('classes', [0, 1], ids=['classes0', 'classes1'])
@cells
def test_r1cs_rows_full_class_coefficients(width, cls, classes):
    """r1cs_row_kernel<W, ASSIGN, CLASSES>: combinations of 1 to 7 products whose coefficients are field elements (fp_dot
    with 1, 2 and 3 products, its rounds of conditional subtractions, the lazy case): assignment, a check that holds, and a
    check after one witness value changed in some lanes"""
    p = mc.modulus(width, cls)
    nb = 4 * width
    pool, levels, checks = r1cs_system(p, width)
    n_lanes = 70
    base = r1cs_values(p, width, n_lanes)
    rows = [r for lvl in levels for r in lvl]
    starts, tv, tc = [], [], []
    for parts in rows + checks:
        for part in parts:
            starts.append(len(tv))
            tv += [v for v, _ in part]
            tc += [c for _, c in part]
    starts.append(len(tv))
    cb = np.frombuffer(b''.join(_le(c, nb) for c in pool), dtype=np.uint8).reshape(len(pool), nb)
    ev = _session(p, [('witness', k) for k in range(R1CS_BASE)], 0, R1CS_BASE, retain_all=True,
                  options=(('r1cs_coef_classes', str(classes)),))
    ev.r1cs_load_csr(np.array(starts, dtype=np.uint32), np.array(tv, dtype=np.uint64), np.array(tc, dtype=np.uint32), cb, nb, len(rows))
    cc = ev.r1cs_class_counts()
    assert cc['full'] > 0 and (classes or cc['unit'] == cc['small'] == 0), cc
    if classes and p > 2 ** 40:      # (every coefficient of a field of a few bits is a small integer)
        assert cc['full'] >= 2 * len(rows), cc
    _run(ev, None, base)
    at = 0
    for lvl in levels:
        ev.r1cs_assign(at, len(lvl))
        at += len(lvl)
    got = ev.r1cs_get_vars(list(range(R1CS_BASE, R1CS_BASE + len(rows))), n_lanes)
    refs = [r1cs_reference(p, pool, levels, checks, base[lane]) for lane in range(n_lanes)]
    for lane in range(n_lanes):
        want = refs[lane][0][R1CS_BASE:]
        assert got[lane] == want, (lane, [r for r in range(len(rows)) if got[lane][r] != want[r]])
    ev.r1cs_check()
    ff, counts = ev.r1cs_results(n_lanes)
    assert counts == (n_lanes, 0) and all(int(x) == zk.NO_FAIL for x in ff)
    # one witness value changed in every third lane (the assigned variables stay): the reference's first failing row
    var = 5
    changed = [list(b) for b in base]
    for lane in range(0, n_lanes, 3):
        changed[lane][var] = (changed[lane][var] + 1) % p
    _run(ev, None, changed)
    ev.r1cs_check()
    ff, counts = ev.r1cs_results(n_lanes)
    want = []
    for lane in range(n_lanes):
        v = changed[lane] + refs[lane][0][R1CS_BASE:]
        want.append(refs[lane][1](v))
    assert [None if int(x) == zk.NO_FAIL else int(x) for x in ff] == want
    n_bad = sum(w is not None for w in want)
    assert all((want[lane] is not None) == (lane % 3 == 0) for lane in range(n_lanes))
    assert counts == (n_lanes - n_bad, n_bad)


@pytest.mark.gpu
@pytest.mark.parametrize('cls', ['top', 'tiny'])
@pytest.mark.parametrize('width', [4, 6, 10, 12, 14])
def test_r1cs_unit_and_small_classes_at_the_other_widths(width, cls):
    """the row shapes of test_gpu_parity.py::test_r1cs_small_coefficient_class_at_its_bounds (255 terms of magnitude
    2^31 - 1 on values p - 1, every sign, full beside small) at the widths its four fields do not reach"""
    import test_gpu_parity
    test_gpu_parity.test_r1cs_small_coefficient_class_at_its_bounds(mc.modulus(width, cls))


# --------------------------------------------------------------------------------------------------------- quotient wires
@pytest.mark.gpu
@cells
def test_quotient_wires(width, cls):
    """r1cs_correction_kernel: q = ((a op b) - out) // p of every add / mul / addc / mulc call of the gate relation, on the
    operand pairs of the gate test ((p - 1, p - 1) among them)"""
    p = mc.modulus(width, cls)
    gates = gate_relation(p, width)
    lanes = gate_lanes(p, width, n_random=2)
    ev = _session(p, gates, 0, 2, retain_all=True)
    ev.r1cs_from_tape(use_correction=True)
    _run(ev, None, lanes)
    kinds, a, b = ev.tape()
    calls = [i for i, k in enumerate(kinds) if int(k) in (1, 2, 3, 4)]
    value_gates = [g for g in gates if g[0] not in ('free', 'assert_zero')]
    assert len(calls) == len(value_gates) - 2 and {int(kinds[i]) for i in calls} == {1, 2, 3, 4}
    got = ev.r1cs_correction_values(calls, len(lanes))
    assert (p - 1, p - 1) in lanes
    for lane, (x, y) in enumerate(lanes):
        wires, _, _ = mc.evaluate_gates(gates, p, [], [x, y])
        want = []
        for g in value_gates[2:]:
            rhs = wires[g[3]] if g[0] in ('add', 'mul') else int.from_bytes(g[3], 'little')
            want.append(mc.ref_quotient('add' if g[0] in ('add', 'addc') else 'mul', wires[g[2]], rhs, p))
        assert got[lane] == want, (lane, [i for i in range(len(want)) if got[lane][i] != want[i]])


# ------------------------------------------------------------------------------------------------ derived field constants
@cells
def test_derived_field_constants(width, cls):
    """what the kernels are launched with (zkgpu_mont_field_params), in exact integers: the engine may ask for more
    subtractions than needed, or leave the lazy path off, but never the other way round"""
    for p in (mc.modulus(width, cls), mc.prime_modulus(width, cls)):
        f = zk.mont_field_params(p)
        R = 1 << (32 * width)
        assert f['nwords'] == width and f['p'] == p
        assert f['n0inv'] == (-pow(p, -1, 1 << 32)) % (1 << 32)
        assert f['r2'] == R * R % p
        assert f['one'] == R % p
        r = mc.rho(p, width)
        for K in (1, 2, 3, 4):
            assert mc.ceil_frac(K * r) <= f['dot_rounds'][K - 1] <= K, (K, f['dot_rounds'])
        if f['lazy_dot3']:
            assert (3 * r + 1) * r < 1 and (3 * r + 1) ** 2 * r < 1
        # ... and the class drives what it is named after
        want = {'tiny': ([1, 1, 1, 1], 1), 'lazy_edge_on': ([1, 1, 1, 2], 1), 'lazy_edge_off': ([1, 1, 1, 2], 0),
                'third': ([1, 1, 2, 2], 0), 'half': ([1, 2, 2, 3], 0), 'two_thirds': ([1, 2, 3, 3], 0), 'top': ([1, 2, 3, 4], 0),
                'top_interior': ([1, 2, 3, 4], 0)}.get(cls)
        if want:
            assert ([mc.ceil_frac(K * r) for K in (1, 2, 3, 4)], f['lazy_dot3']) == want
            assert f['dot_rounds'] == want[0]
    assert zk.mont_field_params(mc.modulus(width, 'n0inv_ff'))['n0inv'] == 0xFFFFFFFF
    assert zk.mont_field_params(mc.modulus(width, 'n0inv_one'))['n0inv'] == 1


def test_field_constants_hook_refuses_what_the_montgomery_path_does_not_take():
    for p in (2, 2 ** 64 - 2, 2 ** 512 + 1):
        with pytest.raises(zk.ZkGpuError):
            zk.mont_field_params(p)


def test_operand_set_holds_the_edges():
    """the operand lists are what the issue asks for: sums of exactly p - 1, p, p + 1 and R - 1, R, R + 1 where two values
    below p reach them, 0xFFFFFFFF words, p - 1 squared"""
    for width in mc.WIDTHS:
        R = 1 << (32 * width)
        for cls in mc.CLASSES:
            p = mc.modulus(width, cls)
            pairs = mc.operand_pairs(p, width)
            assert all(0 <= a < p and 0 <= b < p for a, b in pairs)
            sums = {a + b for a, b in pairs}
            assert {p - 1, p, p + 1} <= sums
            if 2 * (p - 1) >= R + 1:
                assert {R - 1, R, R + 1} <= sums
            assert (p - 1, p - 1) in pairs and (0, 0) in pairs and (R % p, R % p) in pairs
            vals = mc.edge_mont_values(p, width)
            if width > 2 or cls != 'tiny':
                assert any(v & 0xFFFFFFFF == 0xFFFFFFFF and v >> 32 == 0 for v in vals)
            assert len(gate_lanes(p, width)) % 64 not in (0, 63)


@pytest.mark.parametrize('width', [4, 6, 8, 10, 12, 14, 16])
def test_regression_three_subtractions_just_above_two_thirds(width):
    """p = (2 R + 1) / 3: 3 p / R = 2 + 1 / R.  Derived from the top 64 bits of p in floating point, the quotient rounded
    to exactly 2 and dot_rounds[2] came out as 2, one below ceil(3 p / R); it is computed over the words of p now"""
    p = mc.modulus(width, 'two_thirds')
    assert 3 * p == 2 * (1 << (32 * width)) + 1
    assert zk.mont_field_params(p)['dot_rounds'] == [1, 2, 3, 3]
