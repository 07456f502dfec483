"""bench.py --gpus N must launch its own ranks when it was not started by torch.distributed.run (the driver calls it both ways).
CPU rehearsal: --dry-run-cpu runs the same launcher, rendezvous, record gather and max-over-ranks reduction over gloo with
fabricated records; the real N > 1 run differs only in the backend (RCCL) and in where the records come from (the prover)."""
import json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(cmd):
    env = dict(os.environ); env.pop('WORLD_SIZE', None); env.pop('RANK', None); env.pop('LOCAL_RANK', None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_self_launch_two_ranks():
    j = _line([sys.executable, 'bench.py', '--gpus', '2', '--steps', '2', '--warmup', '1', '--dry-run-cpu'])
    assert j['n_gpus'] == 2 and j['dry_run'] and j['gathered_records_equal_per_rank_records'] and j['valid'] is False


def test_under_torch_distributed_run():
    j = _line([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
               '--master-port', str(29700 + os.getpid() % 200), 'bench.py', '--gpus', '2', '--dry-run-cpu'])
    assert j['n_gpus'] == 2 and j['gathered_records_equal_per_rank_records']


def test_single_rank_dry_run():
    j = _line([sys.executable, 'bench.py', '--dry-run-cpu'])
    assert j['n_gpus'] == 1 and j['gathered_records_equal_per_rank_records']


def test_launcher_does_not_hang_when_a_rank_dies():
    """If one rank exits with an error the launcher terminates the others (they would wait in the collective until its time-out) and reports it."""
    import time
    env = dict(os.environ, ZKC_BENCH_TEST_FAIL_RANK='1'); env.pop('WORLD_SIZE', None); env.pop('RANK', None); env.pop('LOCAL_RANK', None)
    t0 = time.time()
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '2', '--dry-run-cpu'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode != 0 and 'rank 1 exited with status 7' in r.stderr and time.time() - t0 < 120


def test_eight_ranks_with_an_uneven_tail():
    """[r4] the driver's largest launch (BASELINE configs[3]: eight ranks) rehearsed on the CPU before an 8-GPU box ever sees it: eight gloo ranks, a census that does not
    divide by eight (ranks 3..7 prove one voter less), the census handed out by one broadcast from rank 0, one step time per rank in the line."""
    env_uneven = dict(os.environ, ZKC_BENCH_TEST_UNEVEN='1')
    env_uneven.pop('WORLD_SIZE', None); env_uneven.pop('RANK', None); env_uneven.pop('LOCAL_RANK', None)
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '8', '--steps', '2', '--warmup', '0', '--batch', '13', '--dry-run-cpu'], cwd=ROOT, env=env_uneven, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])
    assert j['n_gpus'] == 8 and j['voters'] == 8 * 13 - 5 and j['gathered_records_equal_per_rank_records']
    assert len(j['ms_per_step_per_rank']) == 8 and all(t >= 0 for t in j['ms_per_step_per_rank'])


def test_eight_ranks_one_dies():
    import time
    env = dict(os.environ, ZKC_BENCH_TEST_FAIL_RANK='5'); env.pop('WORLD_SIZE', None); env.pop('RANK', None); env.pop('LOCAL_RANK', None)
    t0 = time.time()
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '8', '--dry-run-cpu'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode != 0 and 'rank 5 exited with status 7' in r.stderr and time.time() - t0 < 120


def test_dump_outputs_exact_and_bounded(tmp_path):
    """--dump-outputs: byte arrays come back exactly as float32; past the size limit a fixed seeded sample of rows is kept (the same rows in every array
    of that length, the same rows from run to run) and the files stay under the limit."""
    import numpy as np
    code = ("import importlib.util, sys, numpy as np\n"
            "spec = importlib.util.spec_from_file_location('bench', 'bench.py'); b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)\n"
            "a = (np.arange(4096 * 256) * 7 % 256).astype(np.uint8).reshape(4096, 256); s = np.arange(4096, dtype=np.int32).reshape(4096, 1)\n"
            "b.dump_outputs(sys.argv[1] + '/full', {'proofs': a[:64], 'status': s[:64]})\n"
            "b.DUMP_LIMIT = 1 << 20\n"
            "for d in ('cut1', 'cut2'):\n"
            "    b.dump_outputs(sys.argv[1] + '/' + d, {'proofs': a, 'status': s})\n")
    r = subprocess.run([sys.executable, '-c', code, str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    a = (np.arange(4096 * 256) * 7 % 256).astype(np.uint8).reshape(4096, 256)
    full = {f[:-4]: np.load(tmp_path / 'full' / f) for f in os.listdir(tmp_path / 'full')}
    assert sorted(full) == ['proofs', 'status'] and full['proofs'].dtype == np.float32
    assert (full['proofs'] == a[:64]).all() and (full['status'][:, 0] == np.arange(64)).all()
    cut = tmp_path / 'cut1'
    assert sum(os.path.getsize(cut / f) for f in os.listdir(cut)) <= 1 << 20
    rows = np.load(cut / 'proofs_rows.npy').astype(np.int64)
    assert 0 < len(rows) < 4096 and (np.load(cut / 'status_rows.npy') == rows).all()
    assert (np.load(cut / 'proofs.npy') == a[rows]).all() and (np.load(cut / 'status.npy')[:, 0] == rows).all()
    for f in os.listdir(cut):
        assert (np.load(cut / f) == np.load(tmp_path / 'cut2' / f)).all()


def test_test_key_falls_back_when_the_package_cannot_be_written(tmp_path):
    """bench.py on a checkout it may only read: the seeded test key goes to a per-user directory under the temporary directory instead of failing;
    any other error is not swallowed."""
    code = ("import errno, importlib.util, sys, tempfile\n"
            "spec = importlib.util.spec_from_file_location('bench', 'bench.py'); b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)\n"
            "class S:\n"
            "    def __init__(self, err): self.err, self.calls = err, []\n"
            "    def ensure_test_artifacts(self, nl, directory=None):\n"
            "        self.calls.append(directory)\n"
            "        if directory is None: raise self.err\n"
            "        return directory\n"
            "s = S(PermissionError(errno.EACCES, 'denied')); d = b.test_artifacts(s, 10)\n"
            "assert s.calls == [None, d] and d.startswith(tempfile.gettempdir()), s.calls\n"
            "s = S(OSError(errno.ENOSPC, 'full'))\n"
            "try:\n"
            "    b.test_artifacts(s, 10); raise SystemExit('ENOSPC was swallowed')\n"
            "except OSError as e:\n"
            "    assert e.errno == errno.ENOSPC and s.calls == [None]\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr[-2000:]
