"""The `--gpus 1` headline of bench.py on the HIP engine: a plain run is the
timed VMC leg alone, and `--dump-outputs` writes the state its last timed step
left -- the same from run to run, and the state the oracle evaluates to."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import ROOT

pytestmark = pytest.mark.gpu

# 2^17 chains: more than the 48 MB of positions a dump holds at N = 64, so
# that the dump is a fixed sample of the chains
CHAINS = 1 << 17


def run_plain(outdir):
    env = {k: v for k, v in os.environ.items()
           if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR',
                        'MASTER_PORT', 'QMC_BENCH_BACKEND')}
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
         '--steps', '24', '--warmup', '4', '--pre-equil', '256', '--equil',
         '32', '--chains', str(CHAINS), '--dump-outputs', str(outdir)],
        env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_state_of_the_last_timed_step(oracle, tmp_path):
    from bench import box_spec
    outs, dumps = [], []
    for k in range(2):
        d = tmp_path / f'out{k}'
        outs.append(run_plain(d))
        names = sorted(os.listdir(d))
        assert names == ['vmc_chain.npy', 'vmc_energy.npy', 'vmc_pos.npy',
                         'vmc_wf_abs_log.npy']
        dumps.append({nm[:-4]: np.load(d / nm) for nm in names})
    out = outs[0]
    assert out['metric'] == 'walker-steps/sec' and out['value'] > 0
    assert out['unit'] == 'walker-steps/s' and out['dtype'] == 'f64'
    assert out['higher_is_better'] is True
    assert out['n_gpus'] == 1 and out['steps'] == 24 and out['warmup'] == 4
    assert out['value'] == pytest.approx(CHAINS * 1e3 / out['ms_per_step'])
    # the headline alone: no other leg, no CPU baseline, no windows
    assert 'cpu_baseline' not in out
    assert not {'dmc', 'c4_dmc_sharded', 'vmc_accept_rate'} & set(out['extra'])
    a, b = dumps
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for nm in a:
        assert a[nm].dtype == np.float64
        assert np.array_equal(a[nm], b[nm]), nm
    rows = len(a['vmc_chain'])
    assert rows < CHAINS and a['vmc_pos'].shape == (rows, 64)
    assert a['vmc_wf_abs_log'].shape == a['vmc_energy'].shape == (rows,)
    idx = a['vmc_chain']
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < CHAINS
    # the dumped rows are consistent states: the oracle evaluates the
    # positions to the dumped log |psi| and local energy
    m = oracle.model_from_cfc(box_spec(64).cfc_spec)
    pick = np.linspace(0, rows - 1, 16).astype(int)
    wf, en, _, _ = oracle.evaluate_set(m, a['vmc_pos'][pick])
    assert np.allclose(a['vmc_wf_abs_log'][pick], wf, rtol=1e-9, atol=1e-9)
    assert np.allclose(a['vmc_energy'][pick], en, rtol=1e-9, atol=1e-9)
