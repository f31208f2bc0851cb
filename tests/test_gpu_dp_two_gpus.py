"""Native data parallelism across TWO REAL GPUs (RCCL over xGMI, world 2): runs wherever two devices are visible and is skipped
on the one-GPU test boxes of this project (round-2 advisor: the RCCL path with world > 1 had no test that could ever run).
Each case starts `bench.py --gpus 2 --full` (fresh rank processes; the replica check and the per-launch collective time are
measured under --full) and reads its JSON line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _two_gpus():
    import torch
    return torch.cuda.device_count() >= 2


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'FNN_BENCH_REHEARSE')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '30', '--warmup', '5', '--full', '--no-extras',
                        '--no-cpu-baseline'] + list(extra), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])


@pytest.mark.skipif(not _two_gpus(), reason="needs two GPUs")
@pytest.mark.parametrize("extra", [(), ('--dp-payload', 'bucket'), ('--dp-collective', 'p2p')])
def test_two_ranks_exchange_mode_keeps_replicas_identical(extra):
    """EXCHANGE mode over two GPUs, in each form of the dense collective: every rank's table carries the same checksum after
    the run (each applies the global batch's row updates in global example order; the dense tensors come from one sum)."""
    out = _bench('--dp-sparse', 'exchange', *extra)
    dp = out['data_parallel']
    assert out['n_gpus'] == 2 and dp['native_setup_error'] is None
    assert dp['exact_mode_check']['replicas_identical'] is True
    if '--dp-collective' in extra:
        assert dp['payload'] == 'bucket' and 'p2p' in dp['collective']


@pytest.mark.skipif(not _two_gpus(), reason="needs two GPUs")
def test_two_ranks_local_mode_runs_and_reports_the_collective():
    out = _bench()
    assert out['n_gpus'] == 2 and out['value'] > 0 and out['data_parallel']['collective_us'] > 0
