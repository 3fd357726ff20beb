"""bench.py as the driver runs it: the plain run's one JSON line and what --dump-outputs writes.

CPU: the rows --dump-outputs samples are fixed and bounded.
GPU: a plain run on a small workload prints the headline line only; its dumped outputs are the oracle's state after
exactly W + K iterations, and a second run with the same arguments writes the same bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_rows_are_a_fixed_bounded_sample():
    small = bench.dump_rows(1000)
    assert np.array_equal(small, np.arange(1000))
    n = 10_000_000
    rows = bench.dump_rows(n)
    assert rows.size == bench.DUMP_ROWS and rows.size * 8 * 2 <= 64 << 20
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    assert np.array_equal(rows, bench.dump_rows(n))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    from new_cg_variants_amd import problems
    from oracle import ne_oracle as orc
    K, W = 20, 5

    def run(out):
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(K), '--warmup', str(W),
               '--workload', 's3_small', '--dump-outputs', str(out)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, p.stdout[-2000:]
        return json.loads(lines[0])

    out = tmp_path / 'outputs'
    d = run(out)
    assert d['steps'] == K and d['warmup'] == W and d['unit'] == 'iters/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f64' and d['metric'].startswith('pipe_pr_cg iterations/sec')
    assert d['value'] > 0 and abs(d['ms_per_step'] * d['value'] - 1e3) <= 1e-9 * 1e3
    assert d['config']['residual_finite']
    # the legs of --full stay out of a plain run
    assert d['cpu_baseline'] is None and 'workloads' not in d and d['value_general_csr'] is None
    assert 'spmv' not in d['roofline'] and 'stream_ceiling' not in d['roofline']

    wl = problems.WORKLOADS['s3_small']
    A = wl['make']()
    b, x0, _ = problems.reference_rhs(A, wl['n'])
    assert sorted(os.listdir(out)) == ['r.npy', 'scalars.npy', 'x.npy']
    x, r, s = (np.load(out / f'{name}.npy') for name in ('x', 'r', 'scalars'))
    assert x.dtype == r.dtype == s.dtype == np.float64
    assert x.shape == r.shape == (wl['n'],) and s.shape == (5,)

    # the state after exactly W + K iterations of the oracle's pipe_pr_cg loop, and not the one before or after:
    # the device sums its inner products in another order (x drifts ~1e-11, r ~1e-8, the scalars ~1e-14 from the
    # oracle by then), while one iteration changes x by ~2e-2, r by ~1, the scalars by ~0.2
    st = orc.pipe_start(A, b, x0)
    ref = {}
    for k in range(1, W + K + 2):
        orc.pipe_advance(A, st, 'pr')
        ref[k] = (st.x.copy(), st.r.copy(), np.array([st.mu, st.dl, st.gm, st.nu, np.dot(st.r, st.r)]))

    def close(k):
        rx, rr, rs = ref[k]
        return (np.linalg.norm(x - rx) <= 1e-8 * np.linalg.norm(rx) and np.linalg.norm(r - rr) <= 1e-5 * np.linalg.norm(rr)
                and np.all(np.abs(s - rs) <= 1e-9 * np.abs(rs)))
    assert close(W + K), (s, ref[W + K][2])
    assert not close(W + K - 1) and not close(W + K + 1)

    # the same arguments give the same outputs, bit for bit
    again = tmp_path / 'again'
    run(again)
    for name in ('x', 'r', 'scalars'):
        assert np.array_equal(np.load(again / f'{name}.npy'), np.load(out / f'{name}.npy')), name
