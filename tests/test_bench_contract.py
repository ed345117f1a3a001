"""The bench line contract, checked on the committed line of the latest measured build (profiles/) -- no GPU needed."""
import glob
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def latest_line():
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_bench_v*_final.json')))
    assert files, 'no committed bench line under profiles/'
    return json.load(open(files[-1])), files[-1]


def test_committed_bench_line_has_the_contract_fields():
    d, path = latest_line()
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert key in d, '%s: missing %r' % (path, key)
    assert d['n_gpus'] == 1 and d['higher_is_better'] is True and d['dtype'] == 'f64' and d['data'] == 'synthetic'
    assert d['vs_baseline'] is None                       # BASELINE.json publishes no number
    assert 'workload' in d['config'] and 'model' not in d['config']
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 - 512 * 512 * 256 * 512) <= 1e-6 * 512 * 512 * 256 * 512   # cells x steps x chains of one fit
    r = d['roofline']
    assert (r['bound'], r['unit'], r['peak']) in (('hbm', 'GB/s', 8000.0), ('mfma', 'TFLOP/s', 78.6))
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-12 and 0.0 < r['frac'] < 1.0
    # `achieved` prices the kernel at the bytes it REALLY moves (the state lives in LDS): PMC bytes per logical launch when the
    # profiler ran, else the designed ones; the two agree; the calibrated copy rate is not exceeded
    if r['bound'] == 'hbm':
        assert abs(r['achieved'] - r['bytes_per_cell_step'] * r['cells_per_launch'] / (r['avg_launch_us'] * 1e-6) / 1e9) < 1e-6 * r['achieved']
        designed = r['hbm']['designed_bytes_per_cell_step'] * r['cells_per_launch']
        assert r['traffic'] is None or 0.9 * designed <= r['traffic'] <= 1.1 * designed
    assert r['frac_calibrated'] is None or r['frac_calibrated'] <= 1.0
    # the three fractions keep their names and meanings from round to round (round 2's `frac` was the streaming-equivalent one, round
    # 3's the real-HBM one: the series to compare across rounds is each NAMED field, `frac` is whichever bounds the kernel):
    #   frac_hbm_real        = real HBM bytes (PMC, else by construction) / time / 8 TB/s
    #   frac_fp64            = fp64 flop as executed / time / 78.6 TFLOP/s
    #   frac_streaming_equiv = SURVEY 8(d) bytes (16 forward / 32 backward per cell-step) / time / 8 TB/s -- may exceed 1
    assert abs(r['frac_hbm_real'] - r['hbm']['achieved_GBs'] / 8000.0) < 1e-12
    assert abs(r['frac_fp64'] - r['fp64']['achieved_TFLOPs'] / 78.6) < 1e-12
    assert abs(r['frac_streaming_equiv'] - r['algorithmic']['GBs_equiv'] / 8000.0) < 1e-12
    assert r['frac'] == (r['frac_hbm_real'] if r['bound'] == 'hbm' else r['frac_fp64'])
    # the SURVEY 8(d) streaming-equivalent rate is there for comparison with earlier rounds, under a name of its own
    assert r['algorithmic']['bytes_per_cell_step'] in (16.0, 32.0) and r['algorithmic']['GBs_equiv'] > r['achieved'] * (r['bound'] == 'hbm')
    for p_, v in _walk(d):
        if p_.endswith('achieved_GBs') or (p_.endswith('/achieved') and d['roofline']['unit'] == 'GB/s'):
            assert v <= 8000.0, (p_, v)                   # nothing called "achieved" exceeds the HBM peak
        if p_.endswith('frac_calibrated') and v is not None:
            assert v <= 1.0, (p_, v)
    c = d['cpu_baseline']
    assert c['kind'] == 'port' and c['cores'] >= 1 and c['unit'] == d['unit'] and c['value'] > 0 and c['sample']
    # C5 counts the chains it runs
    if 'c5' in d.get('extra', {}) and 'config' in d['extra']['c5']:
        assert d['extra']['c5']['config']['n_hyper'] == 250


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_module', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_compact_line_of_the_largest_committed_record_fits_the_driver():
    """Round 4's 35 KB line was not parsed by the driver (BENCH_r04.parsed null).  bench.compact_line() of EVERY committed full record
    (the 35 KB one included) stays under 8 KB, is one line, and keeps the contract fields, `roofline` (with frac, traffic, the three
    named fractions, kernel, avg_launch_us, cells_per_launch) and `cpu_baseline`."""
    bench = _bench_module()
    assert bench.LINE_LIMIT <= 8192
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_bench_v*_final.json')))
    biggest = 0
    for f in files:
        full = json.load(open(f))
        if 'roofline' not in full or not isinstance(full.get('kernels'), dict) or 'hbm' not in next(iter(full['kernels'].values()), {}):
            continue                                        # (lines of rounds 1 - 2 predate the per-pass record layout)
        text = bench.compact_line(full)
        biggest = max(biggest, len(text))
        assert len(text) < 8192 and '\n' not in text, (f, len(text))
        d = json.loads(text)
        for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                    'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
            assert key in d, (f, key)
        assert d['value'] == full['value'] and d['ms_per_step'] == full['ms_per_step']         # full precision where the driver reads
        r = d['roofline']
        for key in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'frac_hbm_real', 'frac_fp64', 'frac_streaming_equiv', 'kernel',
                    'avg_launch_us', 'cells_per_launch'):
            assert key in r, (f, key)
        assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-4
        c = d['cpu_baseline']
        assert c['kind'] == 'port' and c['cores'] >= 1 and c['value'] > 0 and c['sample']
        for name, e in d.get('extra', {}).items():
            assert set(e) <= {'value', 'ms_per_step', 'log_evidence_rel_err', 'resident_fallbacks', 'fwd_us', 'bwd_us', 'frac_hbm_real',
                              'frac_streaming_equiv', 'frac_fp64', 'log_evidence_rel_err_per_chain', 'log_evidence_rel_err_bound',
                              'speedup_vs_reference_wall', 'end_to_end_value', 'host_ms', 'kernel_ms', 'error'}, (name, set(e))
    assert biggest > 0


def test_compact_line_survives_a_record_that_is_too_big():
    """Whatever is put into the record, the headline is never lost: side records are dropped (largest first) to stay under the limit."""
    bench = _bench_module()
    full = json.load(open(sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_bench_v*_final.json')))[-1]))
    full['extra'] = {('w%03d' % i): dict(full['extra']['c3']) for i in range(200)} if 'extra' in full and 'c3' in full['extra'] else {}
    text = bench.compact_line(full)
    assert len(text) < 8192
    d = json.loads(text)
    assert d['value'] == full['value'] and d['roofline']['frac'] > 0 and 'cpu_baseline' in d


def test_the_parity_gate_reports_the_user_visible_log_evidence():
    """ADVICE r4 / VERDICT weak #1: `log_evidence_rel_err` means S.logEvidence vs the reference for EVERY workload; a workload whose
    figure may exceed 1e-9 has a registered bound (tests/tolerances.py BENCH_LOG_EVIDENCE_BOUND) that bench.py guards."""
    import tolerances
    bench = _bench_module()
    assert bench.registered_bound('c4') == 1e-9 and bench.registered_bound('c3') == 1e-9
    assert bench.registered_bound('coal_breakpoints') == tolerances.COAL_NOISE_TOL['logE_rtol'] < 1e-4
    src = open(os.path.join(ROOT, 'bench.py')).read()
    assert "['log_evidence_rel_err'] = float(np.max" not in src          # the per-chain maximum lives under its own key


def _walk(d, path=''):
    if isinstance(d, dict):
        for k, v in d.items():
            yield from _walk(v, path + '/' + str(k))
    elif isinstance(d, list):
        for i, v in enumerate(d):
            yield from _walk(v, path + '/%d' % i)
    else:
        yield path, d


def test_roofline_accounting_of_a_resident_pass():
    """bench.roofline_of on a synthetic timing record of the chain-resident kernels (C4: forward 8 B, backward + fold 24 B per
    cell-step by construction): the HBM figures use the REAL bytes, the streaming-equivalent rate is not called `achieved`."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_module', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    units = 512 * 512 * 256 * 512
    timing = dict(forward_ms=93.6, backward_ms=150.5, forward_launches=512, backward_launches=512, fwd_kernel_variant=6,
                  bwd_kernel_variant=6, fwd_hbm_bytes=8.0 * units, bwd_hbm_bytes=24.0 * units, fwd_flops=130.0 * units,
                  bwd_flops=146.0 * units)
    rf = bench.roofline_of(timing, units, peak_cal=5900.0)
    f, b = rf['forward'], rf['backward']
    assert abs(b['hbm']['bytes_per_cell_step'] - 24.0) < 1e-12 and abs(f['hbm']['bytes_per_cell_step'] - 8.0) < 1e-12
    assert abs(b['hbm']['achieved_GBs'] - 24.0 * units / 150.5e-3 / 1e9) < 1e-6
    assert abs(b['streaming_equiv']['GBs_equiv'] - 32.0 * units / 150.5e-3 / 1e9) < 1e-6
    assert b['hbm']['frac_calibrated'] <= 1.0 and f['hbm']['frac_calibrated'] <= 1.0
    assert f['bound'] == 'fp64' and b['bound'] == 'hbm'
    for path, v in _walk(rf):
        if path.endswith('achieved_GBs'):
            assert v <= 8000.0, (path, v)
        assert not path.endswith('/achieved'), path          # per-kernel objects carry no bare `achieved`
    # the PMC bytes, when given, replace the designed ones
    rf2 = bench.roofline_of(timing, units, peak_cal=5900.0,
                            pmc=dict(backward=dict(bytes=23.8 * units / 512, source='pmc')))
    assert abs(rf2['backward']['hbm']['bytes_per_cell_step'] - 23.8) < 1e-9 and rf2['backward']['hbm']['source'] == 'pmc'


def test_kernel_direction_parser():
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_module', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    kd = bench.kernel_direction
    assert kd('void blc::chain_kernel<14, 4, true, false>(blc::ChainParams)') == 'backward'
    assert kd('void blc::chain_kernel<6, 4, false, true>(blc::ChainParams)') == 'forward'
    assert kd('void blr::resident_kernel<128, 128, 32, 8, false, true>(blr::ResParams)') == 'forward'
    assert kd('void blr::resident_kernel<64, 64, 8, 8, true, false>(blr::ResParams)') == 'backward'
    assert kd('void blm::mfma_step_kernel<2, 1, 8, true, false>(blf::FastParams)') == 'backward'
    assert kd('void blc::chain_fold2_kernel<14, 4>(blc::ChainParams)') == 'backward'
    assert kd('void blk::reduce_partials_kernel(double const*, double*, int, int)') is None


def test_c5_counts_the_chains_it_runs():
    """np.arange(3, 1000, 4)[:256] holds 250 candidates (BASELINE.json says 256): `units` and config.n_hyper use the real count."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location('bench_module', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    import bayesloop_amd as bl
    S, kw, units, desc = bench.make_study(bl, 'c5')
    assert desc['n_hyper'] == 250 == len(np.arange(3, 1000, 4)[:256]) and units == 512 * 512 * 1000 * 250


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _check_tiny_line(stdout, n):
    lines = [l for l in stdout.strip().splitlines() if l.strip()]
    d = json.loads(lines[-1])                                  # the ONE JSON line is the LAST line on stdout
    assert len(lines[-1]) < 8192                               # ... and short enough for the driver to parse
    assert sum(1 for l in lines if l.lstrip().startswith('{')) == 1
    assert d['n_gpus'] == n and d['steps'] == 2 and d['warmup'] == 1 and d['scaling'] == 'strong'
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 - 24 * 24 * 10 * 6) < 1e-6 * 24 * 24 * 10 * 6
    assert np.isfinite(d['log_evidence']) and d['config']['n_hyper'] == 6
    return d


def test_bench_py_under_the_drivers_launcher_two_ranks():
    """`python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P bench.py --gpus 2
    --steps K --warmup W` exactly as the driver starts it, on the test doubles (oracle engine + gloo): launcher environment,
    the sharded fit with its ONE gather + ONE reduce, barrier + max-over-ranks timing, rank 0 prints ONE JSON line, last."""
    import subprocess
    import sys
    import pytest
    pytest.importorskip('torch')
    env = dict(os.environ, BLHIP_BENCH_TEST_DOUBLE='1', OMP_NUM_THREADS='1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT', 'MASTER_ADDR'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1',
           '--workload', 'tiny', '--no-extra', '--no-cpu', '--no-pmc']
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d2 = _check_tiny_line(r.stdout, 2)
    # the same workload with one rank gives the same evidence
    r1 = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '2', '--warmup', '1', '--workload', 'tiny',
                         '--no-extra', '--no-cpu', '--no-pmc'], env=env, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-3000:]
    d1 = _check_tiny_line(r1.stdout, 1)
    assert abs(d1['log_evidence'] - d2['log_evidence']) <= 1e-12 * abs(d1['log_evidence'])


def test_bench_py_self_launch_three_ranks():
    """`python bench.py --gpus 3` without a launcher starts its own ranks (RANK / LOCAL_RANK / WORLD_SIZE / a fresh rendezvous
    key per run) and passes rank 0's line through."""
    import subprocess
    import sys
    import pytest
    pytest.importorskip('torch')
    env = dict(os.environ, BLHIP_BENCH_TEST_DOUBLE='1', OMP_NUM_THREADS='1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT', 'MASTER_ADDR'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '3', '--steps', '2', '--warmup', '1',
                        '--workload', 'tiny', '--no-extra', '--no-cpu', '--no-pmc'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    _check_tiny_line(r.stdout, 3)
    # a launcher / --gpus mismatch is refused loudly
    bad = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--workload', 'tiny'],
                         env=dict(env, WORLD_SIZE='3', RANK='0'), capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and 'WORLD_SIZE=3' in (bad.stderr + bad.stdout)


def _run_tiny(*extra, tmp=None):
    import subprocess
    import sys
    env = dict(os.environ, BLHIP_BENCH_TEST_DOUBLE='1', OMP_NUM_THREADS='1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT', 'MASTER_ADDR'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--workload', 'tiny'] + list(extra), env=env, cwd=tmp,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def test_a_plain_run_times_the_steps_it_is_given_and_nothing_else(tmp_path):
    """`bench.py --steps K --warmup W` without --full: K timed steps, the headline fields, no side measurement, no detail file."""
    d, err = _run_tiny('--steps', '4', '--warmup', '0', tmp=str(tmp_path))
    assert d['steps'] == 4 and d['warmup'] == 0
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 - 24 * 24 * 10 * 6) < 1e-6 * 24 * 24 * 10 * 6
    assert (d['metric'], d['unit'], d['higher_is_better'], d['dtype']) == ('grid-cells*timesteps/sec (fit())', 'grid-cells*timesteps/s', True, 'f64')
    for k in ('cpu_baseline', 'extra', 'end_to_end', 'cold_first_fit_ms', 'log_evidence_rel_err', 'detail'):
        assert k not in d, k
    assert d['roofline'] is None and not d['kernels']
    assert 'full record in' not in err                     # (write_detail's note: bench_detail.json is --full's)


def test_dump_outputs_writes_the_last_steps_results_the_same_in_every_run(tmp_path):
    import numpy as np
    a, b = tmp_path / 'a', tmp_path / 'b'
    da, err = _run_tiny('--steps', '2', '--warmup', '1', '--dump-outputs', str(a))
    db, _ = _run_tiny('--steps', '2', '--warmup', '1', '--dump-outputs', str(b))
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {'logEvidence.npy', 'posteriorSequence.npy', 'posteriorMeanValues.npy', 'logEvidenceList.npy'} <= set(names)
    # localEvidence of a full Gaussian fit is NaN throughout (0 / 0 in the backward pass, as in the reference): left out, and said so
    assert 'localEvidence.npy' not in names and 'localEvidence (10 of 10 entries not finite)' in err
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64) and np.all(np.isfinite(x)) and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 * 2 ** 20
    assert float(np.load(a / 'logEvidence.npy')[0]) == da['log_evidence'] == db['log_evidence']
    assert np.load(a / 'posteriorSequence.npy').shape == (10, 24, 24)


def test_full_keeps_the_side_measurements():
    d, err = _run_tiny('--steps', '2', '--warmup', '1', '--full', '--no-extra', '--no-cpu', '--no-pmc', '--no-e2e')
    assert 'full record in' in err and d['detail'] == 'bench_detail.json' and 'cpu_baseline' in d['config'] and 'log_evidence_rel_err' in d
