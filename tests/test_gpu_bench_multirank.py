"""bench.py's N > 1 launch contract on a one-GPU box: two ranks started with torch.distributed.run, both on cuda:0
over gloo (FARNN_BENCH_ONE_DEVICE=1; with one rank per device the same code runs over RCCL).  Checks the single JSON
line rank 0 prints."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


@pytest.mark.parametrize('extra', [[], ['--workload', 'train']])
def test_bench_two_ranks_on_one_device(extra):
    env = dict(os.environ, FARNN_BENCH_ONE_DEVICE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
           '127.0.0.1', '--master-port', str(_free_port()), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '5',
           '--warmup', '2', '--no-cpu-baseline', '--full'] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['steps'] == 5 and d['warmup'] == 2 and d['value'] > 0 and d['scaling'] == 'weak'
    assert d['config']['valid_tokens_per_step'] > 8000          # both ranks' shards are counted
    assert 'roofline' in d and d['roofline']['frac'] > 0


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no torchrun around it (the form the round driver may use): the parent
    starts the two ranks itself, relays ONE JSON line with n_gpus = 2 and both shards counted."""
    env = dict(os.environ, FARNN_BENCH_ONE_DEVICE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '5', '--warmup', '2',
           '--no-cpu-baseline']
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['steps'] == 5 and d['value'] > 0
    assert d['config']['valid_tokens_per_step'] > 2 * 8000
    assert d['config']['padded_tokens_per_step'] == 2 * 256 * 64


def test_bench_refuses_a_world_size_mismatch():
    env = dict(os.environ, FARNN_BENCH_ONE_DEVICE='1', WORLD_SIZE='1', RANK='0', LOCAL_RANK='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2'], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'WORLD_SIZE' in (r.stderr + r.stdout)


def test_bench_default_line_carries_every_single_gpu_config():
    """The default invocation, as the round driver runs it: the LAST stdout line is the ONE result line (<= 4 KB: round 5's
    20 KB line was unparseable) -- headline = configs[1] with a roofline fraction against the ceiling that bounds it (ONE rule,
    fixed before the run: a cache-resident kernel that beats its modelled split says `model_falsified` and is priced at the L2
    gather rate for every byte: no fraction above 1), a post-run oracle check, both CPU baselines; the other single-GPU configs
    are `{"other_config": ...}` lines before it, and everything is in gpurun_out/bench_full.json."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '20', '--warmup', '5', '--full',
                        '--cpu-seconds', '2'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines[-1]) <= 4096 and lines[-1].startswith('{"metric"'), len(lines[-1])
    assert sum(ln.startswith('{"metric"') for ln in lines) == 1
    assert len(r.stdout) < 8000, len(r.stdout)             # the whole of stdout fits the tail the driver keeps
    d = json.loads(lines[-1])
    rf = d['roofline']

    def frac_ok(rf):
        if not 0 < rf['frac'] <= 1.0:
            return False
        if rf['bound'] == 'infinity_cache':              # cache-resident: the stricter reading is the line's `frac` once the split is beaten
            return 0 < rf['frac_all_l2'] <= 1.0 and (rf.get('model_falsified') is not True or rf['frac_split'] > 1.0)
        return True
    assert rf['launches_timed'] >= 8 and frac_ok(rf) and rf['bound'] in ('infinity_cache', 'hbm'), rf
    assert rf['kernel_avg_us'] > 0 and d['steps'] == 20 and d['warmup'] == 5 and d['n_gpus'] == 1
    assert rf['l1_pipeline']['floor_us'] > 0            # the measured bound beside the bandwidth reading; no range assertion: clock-dependent
    assert d['parity']['tags_equal'] is True
    assert d['cpu_baseline']['value'] > 0 and d['cpu_baseline']['cores'] >= 1 and d['cpu_baseline_faithful']['value'] > 0
    others = [json.loads(ln) for ln in lines[:-1]]
    names = [o['other_config'] for o in others]
    assert names == ['ifst_crf', 'ifst_s104', 'ifst_crf_s104', 'decomp', 'decomp_r250_farnn2',
                     'decomp_r250_farnn2_crf', 'decomp_r250_farnn2_crf_bz200_len30', 'decomp_r150_farnn2_crf_s134_bz200_len30', 'fst4', 'synth512_shard_b1024_len128']
    assert list(d['other_configs_ms_per_step']) == names and d['other_configs_parity'] is True
    for o in others:
        assert 'error' not in o, o
        assert o['value'] > 0 and o['parity']['tags_equal'] is True, o
        assert frac_ok(o['roofline']), o['roofline']
    with open(os.path.join(ROOT, 'gpurun_out', 'bench_full.json')) as f:
        full = json.load(f)
    kern = {o['workload']: o['roofline']['kernel'] for o in full['other_configs']}
    assert 'chain_wide_kernel<fused' in kern['ifst_s104']                # the reference's 104-state automata: the wide form, ONE launch
    assert 'chain_viterbi_kernel' not in kern['ifst_crf']                # config 4: two launches (the one-launch form lives in the A/B build)
    assert full['roofline']['l1_pipeline']['cycles_per_workgroup_step'] == 16 * 24 + 71 * 72 * 4 / 64
    assert abs(full['value'] - d['value']) <= 1e-5 * d['value']



def test_bench_plain_run_dumps_what_its_last_step_returned(tmp_path):
    """The plain invocation (no --full): the contract's keys and nothing measured beside the timed steps, and --dump-outputs
    writes the tags the last of the --steps timed steps returned.  Two runs with the same arguments dump the same tags, and
    they are the oracle's for the batch that step tagged (step i runs batch i mod 4, bench.batch_variants)."""
    from oracle import c_port
    from re2nn_seq_amd import synth
    sys.path.insert(0, ROOT)
    import bench
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    steps = 7
    dumps = []
    for run in range(2):
        out = tmp_path / str(run)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '2',
                            '--dump-outputs', str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        assert len(lines) == 1 and lines[0].startswith('{"metric"'), r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d['steps'] == steps and d['warmup'] == 2 and d['n_gpus'] == 1 and d['unit'] == 'tokens/s' and d['dtype'] == 'f32'
        assert d['higher_is_better'] is True and d['value'] > 0 and d['ms_per_step'] > 0
        tok = d['config']['valid_tokens_per_step']
        assert abs(d['value'] * d['ms_per_step'] * 1e-3 - tok) <= 1e-4 * tok      # value = tokens per step / step time
        for k in ('roofline', 'parity', 'cpu_baseline', 'compact', 'pipelined', 'host_inclusive', 'other_configs_ms_per_step', 'full'):
            assert k not in d, k
        assert os.listdir(out) == ['tags.npy']
        tags = np.load(out / 'tags.npy')
        assert tags.dtype == np.float32 and tags.shape == (256, 64)
        assert int((tags == -1).sum()) == d['config']['padded_tokens_per_step'] - tok
        dumps.append(tags)
    assert np.array_equal(dumps[0], dumps[1])
    _, V, S, C = bench.WORKLOADS['ifst']
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, C, np.random.RandomState(1234))
    x, lengths = synth.random_batch(V, 256, 64, np.random.RandomState(4321))
    xs = bench.batch_variants('ifst', x, lengths, 0, 4)
    ref, _, _ = c_port.onehot_ifst_tag(T + W, O, h0, hT, xs[(steps - 1) % 4], lengths, nthreads=8)
    assert np.array_equal(dumps[0], ref.astype(np.float32))

def test_bench_config5_path_two_ranks_dry_run():
    """BASELINE configs[4]'s code path (`--workload synth512`: device-side tensor generation, the S = 512 geometry of the
    ring kernel, per-rank shards, the overlapped gather) on two ranks over gloo, at a reduced vocabulary so that it fits
    beside a second rank on one device.  The first real 8-GPU run must not be this path's first execution."""
    env = dict(os.environ, FARNN_BENCH_ONE_DEVICE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--workload', 'synth512', '--vocab', '400',
           '--batch', '64', '--seqlen', '128', '--steps', '3', '--warmup', '1', '--no-cpu-baseline']
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['value'] > 0 and 'DRY RUN' in d['config']['workload']
    assert d['config']['padded_tokens_per_step'] == 2 * 64 * 128


@pytest.mark.parametrize('extra', [['--workload', 'ifst', '--batch', '32'],
                                   ['--workload', 'ifst', '--batch', '32', '--gather', 'native'],
                                   ['--workload', 'synth512', '--vocab', '200', '--batch', '16', '--seqlen', '128']])
def test_bench_eight_ranks_dry_run(extra):
    """What the driver's `--gpus 8` run executes, on one device over gloo: eight ranks, each its own shard and handle, the
    overlapped gather of eight blocks, max-over-ranks timing, ONE line with every rank's tokens counted and the per-rank spread
    reported.  (Reduced batch / vocabulary so that eight replicas share one GPU; the first real 8-GPU run must not be the first
    execution of this branch.)"""
    env = dict(os.environ, FARNN_BENCH_ONE_DEVICE='1', HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='2')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '8', '--steps', '3', '--warmup', '1',
           '--no-cpu-baseline'] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    B = int(extra[extra.index('--batch') + 1])
    L = 128 if 'synth512' in extra else 64
    assert d['n_gpus'] == 8 and d['value'] > 0 and d['scaling'] == 'weak'
    assert d['config']['padded_tokens_per_step'] == 8 * B * L
    lo, hi = d['config']['valid_tokens_per_rank_min_max']
    assert 0 < lo <= hi and 8 * lo <= d['config']['valid_tokens_per_step'] <= 8 * hi
    assert '8 ranks' in r.stderr
    # the N > 1 line says which gather ran and how many ranks its communicator has (`--gather native` on one device: the
    # loopback communicator -- the code around the collective; on a node of GPUs, farnn_rccl_gather_tags)
    assert d['gather']['comm_count'] == 8
    assert ('loopback' in d['gather']['backend']) == ('native' in extra)


def test_rccl_gather_c_abi_one_rank():
    """The torch-free tag gather (include/farnn_rccl.h) on a communicator of ONE rank -- what a single-GPU box can run: id,
    communicator, an all-gather of int32 tag blocks on a side stream, the balanced-assignment un-permutation on top of it."""
    import torch
    from re2nn_seq_amd import _rccl, dist as fdist
    if not os.path.exists(_rccl.LIB_PATH):
        pytest.skip('libfarnn_rccl.so not built (optional)')
    assert _rccl.lib().farnn_rccl_version() > 0
    comm = _rccl.Communicator(_rccl.unique_id(), 1, 0, 0)
    local = torch.randint(-1, 128, (37, 64), dtype=torch.int32, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = comm.gather_tags(local, stream=side.cuda_stream)
    side.synchronize()
    assert out.shape == (37, 64) and torch.equal(out, local)
    assert comm.count() == 1
    # bench.py --gather native's loop on that communicator: async gathers on the side stream, two blocks in rotation
    og = fdist.OverlappedGather(37, 64, torch.device('cuda', 0), comm=comm)
    for i in range(5):
        blk = og.next_output()
        blk.fill_(i)
        og.submit()
    og.drain()
    assert bool((og.last() == 4).all())
    lengths = torch.randint(1, 65, (37,))
    assign = fdist.balanced_assignment(lengths, 1)
    assert torch.equal(fdist.gather_tags_balanced_native(local, assign, 37, comm), local)
    comm.close()
