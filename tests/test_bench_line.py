"""bench.py's ONE JSON line stays inside what the driver keeps (6 KB) while it carries every workload of the default run:
checked on the committed detail file of the round (profiles/r04_bench_detail.json = everything that run measured, with
--full).  On the GPU: what a plain run does, its --dump-outputs, and --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_compact_line_of_the_committed_run_fits_and_keeps_every_workload():
    import bench
    full = json.load(open(os.path.join(ROOT, 'profiles', 'r04_bench_detail.json')))
    line = bench.compact_line(full, 'profiles/bench_detail_latest.json')
    text = json.dumps(line)
    assert len(text) <= 6144, len(text)
    assert set(line['secondary']) == {'c4', 'c5', 'c5_small', 'structured', 'structured_chained', 'sha256'}
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in line, k
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in line['roofline'], k
    assert 0 < line['roofline']['frac'] <= 1.0
    for name, w in line['secondary'].items():
        assert w['ms_per_step'] > 0 and w['value'] > 0 and w['roofline']['bound'], name
        if name != 'c5_small':      # (a variant of c5: no CPU sample and no first-verdict session of its own)
            assert w['cpu_baseline']['value'] > 0 and w['first_verdict_s'] and w['break_even_batch'], name
    # the committed line is what compact_line makes of the detail file
    committed = json.loads(open(os.path.join(ROOT, 'profiles', 'r04_bench_default.json')).read())
    assert committed['secondary'].keys() == line['secondary'].keys() and committed['value'] == line['value']


def test_step_outputs_are_float64_with_minus_one_for_a_satisfied_lane():
    import bench
    o = bench.step_outputs(np.array([0xFFFFFFFF, 3, 0], dtype=np.uint32), (2, 1), np.array([0, 1, 0], dtype=np.uint32))
    assert sorted(o) == ['counts', 'first_fail', 'lane_flags']
    assert all(a.dtype == np.float64 for a in o.values())
    assert o['first_fail'].tolist() == [-1.0, 3.0, 0.0] and o['counts'].tolist() == [2.0, 1.0]
    assert o['lane_flags'].tolist() == [0.0, 1.0, 0.0]


def _bench(*args, timeout=600):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + [str(a) for a in args],
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_results_and_full_adds_the_rest(tmp_path):
    """A plain run times the steps it is asked for and nothing else; --dump-outputs writes the verdicts of its last step,
    the same from run to run; --full adds the CPU baseline and the first-verdict sessions."""
    from zkinterface_ir_amd import workloads
    small = ['--gpus', 1, '--warmup', 1, '--batch-per-gpu', 128]
    for extra in (['--width', 256, '--depth', 6], ['--workload', 'c5', '--width', 2048]):
        dumps = []
        for k in range(2):
            d = tmp_path / ('%s_%d' % (extra[0], k))
            r = _bench(*(small + extra + ['--steps', 3, '--dump-outputs', d]))
            assert r['steps'] == 3 and r['ms_per_step'] > 0 and 'cpu_baseline' not in r and 'secondary' not in r
            o = {n: np.load(d / (n + '.npy')) for n in ('first_fail', 'counts')}
            assert all(a.dtype == np.float64 for a in o.values())
            assert o['counts'].tolist() == [r['config']['satisfied'], r['config']['failed']] == [workloads.expected_satisfied(128), 2]
            assert ((o['first_fail'] >= 0) == (np.arange(128) % 97 == 0)).all()
            dumps.append(o)
        assert all(np.array_equal(dumps[0][n], dumps[1][n]) for n in dumps[0])
    r = _bench(*(small + ['--width', 256, '--depth', 6, '--steps', 2, '--full']))
    assert r['cpu_baseline']['value'] > 0 and r['config']['first_verdict_s']
