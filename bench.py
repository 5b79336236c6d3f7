#!/usr/bin/env python3
"""bench.py — BASELINE.json metric: MCMC iters/s + ESS/s on theta, GP classification N=4096,
N_imp=256, on 1/2/4/8 MI355X (one process per GPU, chains sharded, no collective on the data path).

Workload (BASELINE.json configs[3]/[2]): synthetic probit GP-classification data (N=4096, D=32,
ARD squared-exponential kernel), APM with elliptical-slice updates of u and random-direction
slice updates of theta (E-SS+RD-SS.ipynb protocol, w=1, max_steps_out=0), ApproxPosteriorIS
estimator with N_imp=256, `--chains` independent chains per GPU advanced in lockstep.
A step = one MCMC transition (u-update + theta-update) of every chain on every GPU.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N

Rank 0 prints one JSON line (contract in the task statement); `roofline` is the dominant kernel
(the f64-MFMA Cholesky trailing update) timed with HIP events on the context's stream over the
timed region. A plain run sets up, warms up, times the region and prints the line; `--full` adds
what takes work of its own after the timed region: the in-run ESS sample (untimed extension of
the chains), the same workload from prior draws, `cpu_baseline` (the CPU restatement of the
reference, oracle/, timed on this host) and the parity check - their keys are null in a plain
run's line. The timed region is the same in both.
"""
import argparse
import json
import types
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, 'auxiliary-pm-mcmc_amd'))

METRIC = BASE_METRIC = 'MCMC iters/sec + ESS/sec on θ, GP-classif N=4096 N_imp=256, 1/2/4/8 GPU'
PEAK_F64_MFMA_TFLOPS = 78.6   # MI355X FP64 matrix, spec (not in MI355X_MICROARCH.md)
PEAK_F32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: FP32 matrix (v_mfma_f32_*_f32)
PEAK_HBM_TBS = 8.0            # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
PEAK_F16_MFMA_TFLOPS = 2516.6  # MI355X_MICROARCH.md: BF16/FP16 matrix ~2.5 PF dense (spec)
# fp16x3 emulation of the fp32 Newton updates: 3 fp16 MFMA flops per
# fp32-equivalent flop, so its fp32-equivalent ceiling is a third of the fp16 peak
PEAK_F16X3_TFLOPS = PEAK_F16_MFMA_TFLOPS / 3


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100, help='timed transitions per chain (ESS/s needs >= 100)')
    ap.add_argument('--warmup', type=int, default=20, help='untimed transitions per chain (burn-in)')
    ap.add_argument('--chains', type=int, default=64, help='chains per GPU')
    ap.add_argument('--n', '--n-data', dest='n', type=int, default=4096)
    ap.add_argument('--d', '--n-features', dest='d', type=int, default=32)
    ap.add_argument('--n-imp', type=int, default=256)
    ap.add_argument('--seed', type=int, default=20151009)
    ap.add_argument('--schedule', choices=('async',), default='async',
                    help='chain scheduling of the batched sampler (auxpm/batched.py)')
    ap.add_argument('--full', action='store_true',
                    help='after the timed region also run what the headline does not need: the '
                         'untimed ESS extension of the chains, the prior-initialised run, the CPU '
                         'baseline and the parity check (--cpu-baseline, --cpu-budget, --parity, '
                         '--ess-min and --ess-burn act only with --full)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the timed region returned (dump_outputs) as DIR/<name>.npy')
    ap.add_argument('--cpu-baseline', type=int, default=1)
    ap.add_argument('--cpu-budget', type=float, default=30.0,
                    help='approximate seconds of CPU work for the baseline sample')
    ap.add_argument('--parity', type=int, default=1,
                    help='after the timed region: GPU theta-/u-calls vs the oracle (and the '
                         "reference's own full-size fixture); exit 3 on a failure")
    ap.add_argument('--ess-min', type=int, default=100,
                    help='post-burn-in transitions per chain for the ESS (untimed extension)')
    ap.add_argument('--cohorts', type=int, default=1,
                    help='split each rank\'s chains into this many device contexts driven by '
                         'their own host threads (Cohorts): one cohort\'s latency-bound Newton '
                         'phases overlap another\'s MFMA-bound posterior factor')
    ap.add_argument('--ess-burn', type=int, default=50,
                    help='transitions discarded from the start of each chain for the ESS '
                         '(at least --warmup)')
    return ap.parse_args()


class Dist(object):
    """One process per GPU. torch.distributed (gloo, on the host) only for the barrier and the
    max/sum reductions of the timing; the chains never exchange data, so no RCCL communicator is
    created (north_star: "no RCCL required" - one failure mode fewer on an 8-GPU node)."""

    def __init__(self, backend='gloo'):
        self.world = int(os.environ.get('WORLD_SIZE', '1'))
        self.rank = int(os.environ.get('RANK', '0'))
        self.local_rank = int(os.environ.get('LOCAL_RANK', '0'))
        self.dist = None
        self.backend = None
        if self.world > 1:
            import torch.distributed as dist
            dist.init_process_group(backend=backend)
            self.dist = dist
            self.backend = backend

    def _t(self, x):
        import torch
        return torch.tensor([float(x)], dtype=torch.float64)

    def barrier(self):
        if self.dist is not None:
            self.dist.barrier()

    def max(self, x):
        if self.dist is None:
            return float(x)
        t = self._t(x)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def sum(self, x):
        if self.dist is None:
            return float(x)
        t = self._t(x)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return float(t.item())

    def all_gather(self, x):
        """(world, *x.shape) float64 array of every rank's x (same shape on every rank)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if self.dist is None:
            return x[None].copy()
        import torch
        t = torch.from_numpy(x.copy())
        out = [torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(out, t)
        return np.stack([o.numpy() for o in out])

    def broadcast(self, x, src=0):
        """rank src's float64 array x (shape known on every rank) on every rank."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if self.dist is None:
            return x
        import torch
        t = torch.from_numpy(x.copy())
        self.dist.broadcast(t, src)
        return t.numpy()

    def close(self):
        if self.dist is not None:
            self.dist.destroy_process_group()


def rank_device(dist):
    """GPU of this rank: LOCAL_RANK (one process per GPU); APM_DEVICE pins every rank to one
    device instead (the 2-rank rehearsal of the N>1 path on a 1-GPU box, tests/test_gpu_dist.py)."""
    return int(os.environ.get('APM_DEVICE', dist.local_rank))


def chain_seed(base, rank):
    """Seed of rank `rank`'s sampler. Each rank's SeedSequence(seed) spawns its chains' host and
    device (Philox) streams; distinct rank seeds give disjoint chain streams (test_bench_dist)."""
    return base + 7919 * rank


_SYNC_DEVICE = [None]


def device_sync():
    """torch.cuda.synchronize() on this rank's GPU (not on device 0 for every rank); the
    library's own calls are synchronous already, this brackets the timed region."""
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize(_SYNC_DEVICE[0])
    except Exception:
        pass


def csrc_sha16():
    """Digest of the HIP/C++ sources of libapm.so (auxiliary-pm-mcmc_amd/csrc, include/apm.h):
    binds a committed PMC profile to the build it was taken of (tools/profile_round.sh)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(REPO, 'auxiliary-pm-mcmc_amd', 'csrc', '*'))) + \
        [os.path.join(REPO, 'include', 'apm.h')]
    for f in files:
        if f.endswith(('.hip', '.cpp', '.h')):
            h.update(os.path.basename(f).encode())
            h.update(open(f, 'rb').read())
    return h.hexdigest()[:16]


def _pmc_file():
    import glob
    files = sorted(glob.glob(os.path.join(REPO, 'profiles', 'r*_pmc_traffic.json')))
    if not files:
        return None, None
    d = json.load(open(files[-1]))
    return d, os.path.relpath(files[-1], REPO)


def pmc_provenance():
    """{source, csrc_sha16 of the profiled build, of this build, stale} for the PMC numbers."""
    d, src = _pmc_file()
    if d is None:
        return None
    prof = d.get('csrc_sha16')
    cur = csrc_sha16()
    return {'source': src, 'profiled_csrc_sha16': prof, 'commit': d.get('commit'),
            'this_csrc_sha16': cur, 'stale': prof != cur}


def pmc_traffic(*kernels):
    """HBM bytes per dispatch of the kernels (dispatch-weighted over the names given: the bench's
    HIP-event timing of a roofline covers all launch variants of one operation) inside the timed
    region, from the newest committed PMC pass of this bench (profiles/r*_pmc_traffic.json,
    written by tools/prof_window.py from separate `rocprofv3 --pmc FETCH_SIZE` / `--pmc
    WRITE_SIZE` runs of the same command, with the guide's gfx950 corrections). PMC counters
    cannot be read live inside this process."""
    d, src = _pmc_file()
    if d is None:
        return None, None
    d = d.get('pmc_traffic', {})
    tot = n = 0
    for k in kernels:
        e = d.get(k, {})
        b = e.get('traffic_bytes_per_dispatch')
        if b is not None:
            cnt = e['FETCH_SIZE']['dispatches']
            tot += b * cnt
            n += cnt
    if not n:
        return None, None
    return tot / n, src


# flops one MFMA busy cycle of one SIMD performs (MI355X_MICROARCH.md: v_mfma_f64_16x16x4_f64 at
# 32 FLOP/clk/SIMD, v_mfma_f32_16x16x4_f32 at 64, v_mfma_f32_16x16x32_f16 at 1024; fp16x3 counts a
# third of its f16 flops as fp32-equivalent)
MFMA_FLOPS_PER_BUSY_CYCLE = {'f64': 32.0, 'f32': 64.0, 'f16x3': 1024.0 / 3}


def pmc_mfma(kind, *kernels):
    """MFMA utilisation of the kernels (SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE
    / 8), dispatch-weighted) and the flops per dispatch those busy cycles imply, from the newest
    committed PMC pass of this bench (profiles/r*_pmc_traffic.json 'pmc_mfma', written by
    tools/prof_window.py). Counter runs serialise dispatches, so the utilisation is the kernel's
    own, without the concurrent chol(K) stream."""
    d, src = _pmc_file()
    if d is None:
        return None
    d = d.get('pmc_mfma', {})
    busy = act = n = 0.0
    for k in kernels:
        e = d.get(k)
        if e:
            busy += e['mfma_busy_cycles']
            act += e['grbm_gui_active']
            n += e['dispatches']
    if not n or not act:
        return None
    return {'util': busy / (1024.0 * act / 8.0), 'dispatches': int(n),
            'counter_flops_per_launch': busy / n * MFMA_FLOPS_PER_BUSY_CYCLE[kind],
            'source': src}


def timed_region(dist, step_fn, steps, on_start=None):
    """barrier + sync, K steps, barrier + sync; returns the max over ranks of the wall time."""
    dist.barrier()
    device_sync()
    t0 = time.perf_counter()
    if on_start is not None:
        on_start()
    for _ in range(steps):
        step_fn()
    device_sync()
    dist.barrier()
    return dist.max(time.perf_counter() - t0)


def _blas_threads():
    try:
        from threadpoolctl import threadpool_info
        return max([i.get('num_threads', 1) for i in threadpool_info()
                    if i.get('user_api') == 'blas'] or [1])
    except Exception:
        return None


def cpu_baseline(X, y, n_imp, theta, calls_theta, calls_u, budget, U1, U2, min_theta_calls=3):
    """Time the CPU restatement (oracle/: C Gram + scipy LAPACK, the reference's op order) on a
    bounded sample: >= 3 theta-calls (draws U1) and cached u-calls (draws U2) at the benchmark
    size, composed into transitions/s of ONE chain with the per-transition call counts measured
    on the GPU run; plus configs[0] (PM-MH, iso kernel, N=768 D=8, N_imp=1: one theta-call per
    MH iteration), the reference's own CPU configuration. The port/reference calibration ratio
    measured in the build container (tools/cpu_calibration.py -> profiles/r*_cpu_calibration.json)
    is attached. Also returns the first call pair's values: the oracle side of the parity check
    at theta (the timing does not depend on which values are kept)."""
    import glob
    import apm_oracle as orc
    from gpdemo.utils import synthetic_gp_data
    blas_threads = _blas_threads()
    est = orc.ISEstimatorCPU(X, y, orc.make_kernel_func('ard', 1e-8, impl='c'))
    t_theta, t_u = [], []
    first = None
    t_start = time.perf_counter()
    while len(t_theta) < min_theta_calls or (time.perf_counter() - t_start < budget
                                             and len(t_theta) < 8):
        ops0 = est.n_cubic_ops
        t0 = time.perf_counter()
        v1, cache = est(U1, theta)
        t1 = time.perf_counter()
        v2, _ = est(U2, None, cache)
        t2 = time.perf_counter()
        t_theta.append(t1 - t0)
        t_u.append(t2 - t1)
        if first is None:
            first = (v1, v2, est.n_cubic_ops - ops0, np.array(cache[2]))
    tt, tu = float(np.median(t_theta)), float(np.median(t_u))
    per_transition = calls_theta * tt + calls_u * tu
    # configs[0]: PM-MH iso N=768 D=8 N_imp=1 (Pseudo-Marginal MH.ipynb protocol)
    X1, y1 = synthetic_gp_data(768, 8, 20151009, 'iso')
    est1 = orc.ISEstimatorCPU(X1, y1, orc.make_kernel_func('iso', 1e-8, impl='c'))
    th1 = np.r_[0.0, np.log(np.sqrt(8.))]
    t_c1 = []
    for r in range(5):
        ns1 = np.random.RandomState(r).normal(size=(768, 1))
        t0 = time.perf_counter()
        est1(ns1, th1)
        t_c1.append(time.perf_counter() - t0)
    cores_visible = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') \
        else os.cpu_count()
    cal_files = sorted(glob.glob(os.path.join(REPO, 'profiles', 'r*_cpu_calibration.json')))
    cal = None
    if cal_files:  # port/reference ratio measured in the build container (both on its cores)
        c = json.load(open(cal_files[-1]))
        c2 = c['configs2']
        per_tr = lambda k: (calls_theta * c2[k]['theta_call_s'] +  # noqa: E731
                            calls_u * c2[k]['u_call_s'])
        cal = {'source': os.path.relpath(cal_files[-1], REPO), 'host': c['host'],
               'blas_threads': c['blas_threads'],
               'ratio_port_over_reference_per_transition': per_tr('port') / per_tr('reference'),
               'ratio_theta_call': c2['ratio_port_over_reference_theta_call'],
               'ratio_u_call': c2['ratio_port_over_reference_u_call'],
               'reference_theta_call_s': c2['reference']['theta_call_s'],
               'reference_u_call_s': c2['reference']['u_call_s'],
               'configs0_ratio': c['configs0']['ratio_port_over_reference'],
               'configs0_reference_iters_per_s': c['configs0']['reference']['iters_per_s']}
    out = {
        'value': 1.0 / per_transition, 'unit': 'transitions/s (1 chain)',
        'cores': blas_threads if blas_threads else cores_visible, 'kind': 'port',
        'cores_note': ('BLAS threads = the CPU share this process is given (OMP_NUM_THREADS={0}); '
                       '{1} cores are visible to the process but belong to the whole host'
                       .format(os.environ.get('OMP_NUM_THREADS', 'unset'), cores_visible)),
        'sample': ('{0} theta-calls (median {1:.2f} s) and {0} cached u-calls (median {2:.3f} s) '
                   'of the oracle ApproxPosteriorIS (C Gram 1 thread + scipy/OpenBLAS {3} '
                   'threads) at N={4} D={5} N_imp={6}, composed with {7:.2f} theta-calls + '
                   '{8:.2f} u-calls per transition measured on the GPU run'
                   .format(len(t_theta), tt, tu, blas_threads, X.shape[0], X.shape[1], n_imp,
                           calls_theta, calls_u)),
        'theta_call_s': tt, 'u_call_s': tu, 'theta_calls_timed': len(t_theta),
        'theta_call_s_all': t_theta,
        'configs0_pmmh': {'iters_per_s': 1.0 / float(np.median(t_c1)),
                          'sample': '5 theta-calls (fresh u each, as one PM-MH iteration) of the '
                                    'oracle ApproxPosteriorIS, iso kernel, N=768 D=8 N_imp=1 '
                                    '(Pima-shaped synthetic data)',
                          'theta_call_s_median': float(np.median(t_c1))},
        'calibration': cal,
    }
    return out, first


# ------------------------------------------------------------------------------------ parity
# After the timed region every rank evaluates, on its own GPU, one batched theta-call and one
# cached u-call at two thetas (the bench theta*, and a long length-scale) on fixed draws, and
# rank 0 compares them with the oracle (oracle/apm_oracle.py, estimators.py:152-241 in the
# reference's op order) on the same inputs - and with the reference's own outputs at this size
# (tests/golden/config2_ref.npz, made by tests/golden/make_golden_fullsize.py) when its data are
# the bench's. A failed check makes bench.py exit 3 after printing its line.
PARITY_TOL_NATS = 5e-4    # |d log f| of a theta-call / cached u-call
PARITY_FPOST_REL = 1e-8   # max |d f_post| / max |f_post| (fp64-refined Newton modes)
PARITY_U_SEED = 5         # U1, U2: the first two (N, S) normal draws of RandomState(5)
REF_FIXTURE = os.path.join(REPO, 'tests', 'golden', 'config2_ref.npz')


# the headline's regime in the parity block: one of the long-chain record's stationary chain
# states (tests/golden/stationary_thetas.npy row 45, log sigma 3.11: 10 cubic ops per theta-call
# in the reference), row 4 of the reference fixture (make_golden_fullsize.py config2_stationary)
PARITY_STATIONARY_ROW, PARITY_STATIONARY_FIXTURE_ROW = 45, 4


def parity_inputs(n, d, s):
    """The parity thetas, their rows in the reference fixture, and the draws U1, U2."""
    base = np.log(np.sqrt(d))
    thetas = [np.r_[0.0, np.full(d, base)],          # theta* (cpu_baseline's theta)
              np.r_[1.0, np.full(d, base + 2.0)]]    # long length-scale
    rows = [0, 1]
    st = np.load(os.path.join(REPO, 'tests', 'golden', 'stationary_thetas.npy'))
    if st.shape[1] == d + 1:  # (the bench's ARD dimension)
        thetas.append(st[PARITY_STATIONARY_ROW].astype(np.float64))
        rows.append(PARITY_STATIONARY_FIXTURE_ROW)
    rng = np.random.RandomState(PARITY_U_SEED)
    return np.stack(thetas), rows, rng.normal(size=(n, s)), rng.normal(size=(n, s))


def device_counters(ctx):
    """The context's bounded-spin exits and precision fallbacks since its last reset (DESIGN.md
    §3.1, §9): [fp64 Newton reruns, refinement steps, dataflow-panel spin timeouts, TRSV spin
    timeouts, fp64 posterior-bottom reruns] - a chain that timed out is rerun in fp64 or
    reported failed, never returned as a wrong value with status 0 (tests/test_gpu_errors.py)."""
    from gpdemo import _native
    _, rerun, refine = ctx.prof_read(_native.PROF_STATS, reset=True)
    _, df_to, _ = ctx.prof_read(_native.PROF_DF_TIMEOUTS, reset=True)
    _, trsv_to, _ = ctx.prof_read(_native.PROF_TRSV_TIMEOUTS, reset=True)
    _, post64, _ = ctx.prof_read(_native.PROF_POST64_RERUNS, reset=True)
    return np.array([rerun, refine, df_to, trsv_to, post64], dtype=np.float64)


COUNTER_NAMES = ('newton_fp64_reruns', 'newton_refinement_steps', 'dataflow_spin_timeouts',
                 'trsv_spin_timeouts', 'posterior_bottom_fp64_reruns')


def gpu_parity(X, y, n_imp, thetas, U1, U2, device):
    """This rank's GPU values: batched theta-call (U1) + cached u-call (U2) at every theta, and
    the parity context's device counters (device_counters)."""
    from gpdemo import _native
    B = thetas.shape[0]
    ctx = _native.Context(X, y, _native.KERNEL_ARD, 1e-8, n_imp, max_batch=B, n_slots=B,
                          n_ubufs=2, device=device)
    try:
        ctx.u_upload(0, U1)
        ctx.u_upload(1, U2)
        v1, st1, nops = ctx.theta_eval(_native.EST_IS, thetas, [0] * B, list(range(B)))
        v2, st2 = ctx.u_eval(list(range(B)), [1] * B)
        fpost = np.stack([ctx.slot_read(b)[1] for b in range(B)])
        ctrs = device_counters(ctx)
    finally:
        ctx.close()
    return (v1, v2, nops.astype(np.float64), np.maximum(st1, st2).astype(np.float64), fpost,
            np.r_[st1, st2].astype(np.float64), ctrs)


def reference_fixture(X, y, n, d, s, seed):
    """The reference's outputs at this workload (None when absent or another workload); the
    bench's X must hash to the fixture's digest and its y equal the stored y."""
    import hashlib
    if not os.path.exists(REF_FIXTURE):
        return None, 'absent'
    z = np.load(REF_FIXTURE, allow_pickle=False)
    if (int(z['n']), int(z['d']), int(z['s']), int(z['data_seed']), int(z['u_seed'])) != \
            (n, d, s, seed, PARITY_U_SEED):
        return None, 'another workload'
    dig = hashlib.sha256(np.ascontiguousarray(X, dtype=np.float64).tobytes()).hexdigest()
    if dig != str(z['x_sha256']) or not np.array_equal(z['y'].astype(np.float64), y):
        return None, 'data differ on this host (X digest or y)'
    return z, 'ok'


def parity_check(dist, X, y, a, thetas, fix_rows, U1, U2, oracle_first):
    """GPU (every rank) vs oracle (rank 0, broadcast) and vs the reference fixture."""
    import apm_oracle as orc
    B, n = thetas.shape[0], X.shape[0]
    errors = []
    # an exception on one rank must not leave the others waiting in a collective: it is
    # recorded, NaN stands in for the values, and the check fails
    try:
        g1, g2, gops, gst, gf, gst12, gctr = gpu_parity(X, y, a.n_imp, thetas, U1, U2,
                                                        rank_device(dist))
    except Exception as e:  # noqa: BLE001
        errors.append('rank {0} GPU: {1!r}'.format(dist.rank, e))
        g1 = g2 = gops = np.full(B, np.nan)
        gst = np.full(B, -1.0)
        gst12 = np.full(2 * B, -1.0)
        gctr = np.full(len(COUNTER_NAMES), np.nan)
        gf = np.full((B, n), np.nan)
    orc_vals = np.zeros((B, 3))
    orc_f = np.zeros((B, n))
    t_orc = 0.
    if dist.rank == 0:
        t0 = time.perf_counter()
        try:
            est = orc.ISEstimatorCPU(X, y, orc.make_kernel_func('ard', 1e-8, impl='c'))
            for b in range(B):
                if b == 0 and oracle_first is not None:  # cpu_baseline's first call pair
                    v1, v2, ops, f = oracle_first
                else:
                    ops0 = est.n_cubic_ops
                    v1, cache = est(U1, thetas[b])
                    v2, _ = est(U2, None, cache)
                    ops, f = est.n_cubic_ops - ops0, cache[2]
                orc_vals[b] = (v1, v2, ops)
                orc_f[b] = f
        except Exception as e:  # noqa: BLE001
            errors.append('oracle: {0!r}'.format(e))
            orc_vals[:] = np.nan
            orc_f[:] = np.nan
        t_orc = time.perf_counter() - t0
    orc_vals = dist.broadcast(orc_vals)
    orc_f = dist.broadcast(orc_f)
    fscale = np.abs(orc_f).max(1)
    mine = np.concatenate([g1 - orc_vals[:, 0], g2 - orc_vals[:, 1], gops - orc_vals[:, 2], gst,
                           np.abs(gf - orc_f).max(1) / fscale, g1, g2, gst12, gctr])
    allr = dist.all_gather(mine)  # (world, 9B + counters)
    d1, d2, dops, st, frel = (allr[:, k * B:(k + 1) * B] for k in range(5))
    # per rank: every value, status and device counter of its own parity context, so that a
    # failure names the rank, the theta and the path (round-4 verdict: an intermittent 2-rank
    # failure whose block was lost to a truncated log)
    per_rank = []
    for r in range(allr.shape[0]):
        row = allr[r]
        ctr = row[9 * B:]
        per_rank.append({
            'rank': r, 'd_theta_call': row[:B].tolist(), 'd_u_call': row[B:2 * B].tolist(),
            'd_n_cubic_ops': row[2 * B:3 * B].tolist(), 'f_post_max_rel': row[4 * B:5 * B].tolist(),
            'status_theta_call': row[7 * B:8 * B].astype(int).tolist(),
            'status_u_call': row[8 * B:9 * B].astype(int).tolist(),
            'device_counters': {k: (None if np.isnan(v) else int(v))
                                for k, v in zip(COUNTER_NAMES, ctr)}})
    out = {'thetas': ['theta* (log sigma 0, log tau_k log sqrt(D))',
                      'long length-scale (log sigma 1, log tau_k log sqrt(D) + 2)',
                      'stationary chain state (tests/golden/stationary_thetas.npy row {0}, log '
                      'sigma {1:.2f})'.format(PARITY_STATIONARY_ROW, thetas[-1][0])][:B],
           'draws': 'U1, U2 = first two (N, N_imp) normal draws of RandomState({0}); theta-call '
                    'on U1, cached u-call on U2'.format(PARITY_U_SEED),
           'checked_ranks': int(dist.world),
           'd_theta_call': float(np.abs(d1).max()), 'd_u_call': float(np.abs(d2).max()),
           'd_theta_call_per_theta': np.abs(d1).max(0).tolist(),
           'd_u_call_per_theta': np.abs(d2).max(0).tolist(),
           'n_cubic_ops_equal': bool((dops == 0).all()),
           'status_ok': bool((st == 0).all()),
           'f_post_max_rel': float(frel.max()),
           'tol': {'abs_nats': PARITY_TOL_NATS, 'f_post_rel': PARITY_FPOST_REL},
           'oracle': {'theta_call': orc_vals[:, 0].tolist(), 'u_call': orc_vals[:, 1].tolist(),
                      'n_cubic_ops': orc_vals[:, 2].astype(int).tolist(),
                      'seconds': t_orc if dist.rank == 0 else None},
           'per_rank': per_rank}
    n_err = dist.sum(len(errors))
    if errors:
        out['errors'] = errors
    ok = (n_err == 0 and out['d_theta_call'] <= PARITY_TOL_NATS and
          out['d_u_call'] <= PARITY_TOL_NATS and out['n_cubic_ops_equal'] and out['status_ok'] and
          out['f_post_max_rel'] <= PARITY_FPOST_REL)
    z, why = reference_fixture(X, y, a.n, a.d, a.n_imp, a.seed)
    ref = {'fixture': os.path.relpath(REF_FIXTURE, REPO), 'used': z is not None, 'why': why}
    if z is not None:
        have = [r for r in fix_rows if r < z['thetas'].shape[0]]
        if len(have) < B or not np.array_equal(z['thetas'][have], thetas):
            z, why = None, 'fixture rows {0} hold other thetas'.format(fix_rows)
    if z is not None:
        gv1 = allr[:, 5 * B:6 * B]
        gv2 = allr[:, 6 * B:7 * B]
        r1, r2 = z['logf1'][fix_rows], z['logf2'][fix_rows]
        rf = z['f_post'][fix_rows]
        ref.update({
            'reference_theta_call': r1.tolist(), 'reference_u_call': r2.tolist(),
            'd_theta_call': float(np.abs(gv1 - r1).max()),
            'd_u_call': float(np.abs(gv2 - r2).max()),
            'fixture_rows': list(fix_rows),
            'n_cubic_ops_equal': bool((orc_vals[:, 2] == z['n_cubic_ops'][fix_rows]).all() and
                                      (dops == 0).all()),
            'oracle_minus_reference': {
                'theta_call': float(np.abs(orc_vals[:, 0] - r1).max()),
                'u_call': float(np.abs(orc_vals[:, 1] - r2).max()),
                'f_post_max_rel': float((np.abs(orc_f - rf).max(1) /
                                         np.abs(rf).max(1)).max())}})
        # the GPU's f_post vs the reference's: oracle's (checked above) within its own pin
        ok = ok and ref['d_theta_call'] <= PARITY_TOL_NATS and \
            ref['d_u_call'] <= PARITY_TOL_NATS and ref['n_cubic_ops_equal']
    ref['used'] = z is not None
    ref['why'] = why
    out['vs_reference'] = ref
    out['pass'] = bool(ok)
    return out


def ess_block(dist, smp, series, done, burn, elapsed, P):
    """ESS on theta per the reference's analysis protocol (Analyse
    results.ipynb:138-141, coda effectiveSize / gelman.diag restated in auxpm/diagnostics.py):
    each live chain's series after `burn` discarded transitions (>= ess-min of them, the chain
    extended untimed past the timed region where needed); ESS per transition = min over the
    theta components of ESS / length; ess_per_sec = sum over chains of that x the chain's timed
    transitions / the timed wall time (= ESS per transition x transitions/s). R-hat over this
    rank's chains on their common length."""
    from auxpm.diagnostics import effective_size, gelman_rubin
    live = [c for c in range(smp.n_chains) if not smp.failed[c] and len(series[c]) > burn + 3]
    e_min, e_mean, lens = [], [], []
    for c in live:
        x = np.array(series[c][burn:])
        e = effective_size(x)
        e_min.append(e.min() / len(x))
        e_mean.append(e.mean() / len(x))
        lens.append(len(x))
    w = np.array([done[c] for c in live], dtype=np.float64)
    ess_ps = dist.sum(float(np.dot(e_min, w))) / elapsed
    ess_mean_ps = dist.sum(float(np.dot(e_mean, w))) / elapsed
    n_chains = dist.sum(len(live))
    rhat = None
    if len(live) >= 2:
        L = min(lens)
        r = gelman_rubin(np.stack([np.array(series[c][burn:burn + L]) for c in live]))
        rhat = {'max': dist.max(float(r.max())), 'median_rank0': float(np.median(r)),
                'length': int(L), 'chains_per_rank': len(live)}
    return {'ess_per_sec': ess_ps, 'ess_mean_per_sec': ess_mean_ps, 'rhat': rhat,
            'sample': {
                'chains': int(n_chains),
                'burn_in_discarded': int(burn),
                'post_burn_transitions_per_chain_min': int(-dist.max(-min(lens or [0]))),
                'post_burn_transitions_per_chain_max': int(dist.max(max(lens or [0]))),
                'ess_per_transition_mean': dist.sum(float(np.sum(e_min))) / max(1., n_chains),
                'method': 'coda effectiveSize restatement (auxpm/diagnostics.py) per chain on '
                          'its series after the burn-in (warm-up + timed + untimed extension '
                          'transitions of the same chain), min over the {0} theta components, '
                          'divided by the series length; x the chain\'s timed transitions, '
                          'summed over chains and ranks, / timed wall time. R-hat: coda '
                          'gelman.diag restatement, max over components (and ranks)'.format(P)}}


STATIONARY_DATA_SEED = 20151009  # the long-chain record's data (tools/ess_long.py)


def stationary_states(a, P):
    """Start states of the headline run: the long-chain record's chain states (profiles/
    r*_stationary_thetas.npy: 64 chains of this workload after 9000 transitions each, where the
    posterior puts them - log sigma ~3.5, 7-8 Newton iterations per theta-call), so that the timed
    transitions are the stationary ones that a whole chain is made of (the reference times whole
    10 000-transition chains, E-SS+RD-SS.ipynb:203-205). Chain c starts from state c mod 64; u is
    drawn fresh. (None, why) for another workload: the run then starts from prior draws."""
    import glob
    files = sorted(glob.glob(os.path.join(REPO, 'profiles', 'r*_stationary_thetas.npy')))
    if not files:
        return None, 'no stationary-state record'
    if (a.n, a.d, a.n_imp, a.seed) != (4096, 32, 256, STATIONARY_DATA_SEED):
        return None, 'the record belongs to another workload'
    th = np.load(files[-1], allow_pickle=False)
    if th.ndim != 2 or th.shape[1] != P:
        return None, 'record shape {0} does not fit theta of length {1}'.format(th.shape, P)
    return th[np.arange(a.chains) % th.shape[0]].astype(np.float64), \
        os.path.relpath(files[-1], REPO)


def ess_long_record(value, a):
    """The long-chain ESS record of this workload (SURVEY.md §8d protocol, Analyse
    results.ipynb:138-141: R-hat and ESS on long chains after a warm-up; tools/ess_long.py on one
    MI355X -> the newest profiles/r*_ess_long.json): its ESS per transition (min and mean over the
    theta components) x `value`, this run's driver-timed transitions/s from the record's own
    stationary states (ess_per_sec_estimate: the headline), beside the record's own sampling
    rate (ess_per_sec_record, a builder-run number)."""
    import glob
    files = sorted(glob.glob(os.path.join(REPO, 'profiles', 'r*_ess_long.json')))
    if not files:
        return None
    r = json.load(open(files[-1]))
    cfg = r.get('config', {})
    if (cfg.get('n_data'), cfg.get('n_features'), cfg.get('n_imp')) != (a.n, a.d, a.n_imp):
        return None
    ept = r['ess_per_transition_min_component']
    eptm = r.get('ess_per_transition_mean_component')
    # the record's own sampling rate at stationarity (its chains sit where the posterior puts
    # them, log sigma ~3.5 here: ~9 Newton iterations per theta-call against ~4 for this run's
    # prior-initialised chains), on the newest library it ran on
    lib = r.get('latest_library') or {}
    tps_st = lib.get('transitions_per_s') or r.get('transitions_per_s_sampling')
    return {'source': os.path.relpath(files[-1], REPO),
            'ess_per_transition_min_component': ept,
            'ess_per_transition_mean_component': eptm,
            'stationary_transitions_per_s': tps_st,
            'stationary_library_sha16': lib.get('sha16'),
            'stationary_posterior_mean_log_sigma': r.get('posterior_mean_log_sigma'),
            'ess_per_sec_record': ept * tps_st if tps_st else None,
            'ess_mean_per_sec_record': eptm * tps_st if tps_st and eptm is not None else None,
            'ess_per_sec_estimate': ept * value,
            'ess_mean_per_sec_estimate': eptm * value if eptm is not None else None,
            'rhat_max': r['rhat_max'], 'rhat_median': r.get('rhat_median'),
            'converged_rhat_below_1p1': r['rhat_max'] < 1.1,
            'rhat_below_1p1_at_transitions_per_chain':
                r.get('rhat_below_1p1_at_transitions_per_chain'),
            'chains': cfg.get('chains'),
            'warmup_discarded': r.get('warmup_discarded', cfg.get('warmup_discarded')),
            'kept_per_chain': r.get('kept_per_chain', cfg.get('kept_per_chain')),
            'note': 'ESS per transition from the long-chain record x this run\'s driver-timed '
                    'transitions/s from the record\'s stationary states (ess_per_sec_estimate, '
                    'the headline ess_per_sec) or x the record\'s own sampling rate '
                    '(ess_per_sec_record)'}


class Cohorts(object):
    """The rank's chains as K cohorts of n_chains / K chains, each its own sampler and device
    context (own HIP streams) advanced by its own host thread (ctypes calls release the GIL), so
    that the GPU overlaps one cohort's latency-bound Newton phases (TRSVs, dataflow diagonal
    chains, host round trips) with another's MFMA-bound work. Cohort q holds chains
    [q C, (q + 1) C) with the streams of those chains of one n_chains sampler (first_chain), so
    every chain's trajectory is the one it has in a single batch (batch invariance,
    tests/test_gpu_batched.py). Presents the sampler interface bench.py uses."""

    def __init__(self, make, n_chains, k):
        import threading
        self.threading = threading
        self.k = k
        self.C = n_chains // k
        self.parts = [make(self.C, q * self.C) for q in range(k)]
        self.n_chains = n_chains
        self.P = self.parts[0].P

    def _par(self, fn):
        out = [None] * self.k
        err = []

        def run(q):
            try:
                out[q] = fn(q, self.parts[q])
            except BaseException as e:  # noqa: BLE001
                err.append(e)
        ths = [self.threading.Thread(target=run, args=(q,)) for q in range(self.k)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        if err:
            raise err[0]
        return out

    def initialise(self, theta_init=None):
        self._par(lambda q, s: s.initialise(
            None if theta_init is None else theta_init[q * self.C:(q + 1) * self.C]))

    def run_async(self, n_steps, keep_going=False):
        n = np.broadcast_to(np.asarray(n_steps, dtype=np.int64), (self.n_chains,))
        res = self._par(lambda q, s: s.run_async(n[q * self.C:(q + 1) * self.C], keep_going))
        return [t for r in res for t in r[0]], np.concatenate([r[1] for r in res])

    @property
    def failed(self):
        return np.concatenate([s.failed for s in self.parts])

    @property
    def ctxs(self):
        return [s.ctx for s in self.parts]

    def __getattr__(self, name):  # counters and records summed / concatenated over cohorts
        parts = self.__dict__.get('parts')
        if parts is None:
            raise AttributeError(name)
        if name in ('n_theta_calls', 'n_u_calls'):
            return sum(getattr(s, name) for s in parts)
        if name == 'call_ops':
            return [o for s in parts for o in s.call_ops]
        if name == 'wall':
            return {k: sum(s.wall[k] for s in parts) for k in parts[0].wall}
        raise AttributeError(name)

    def reset_records(self):
        for s in self.parts:
            s.call_ops = []
            for k in s.wall:
                s.wall[k] = 0.
            for h in s.ctx.batch_hist.values():
                h.clear()

    def batch_hist(self):
        out = {}
        for s in self.parts:
            for kind, h in s.ctx.batch_hist.items():
                d = out.setdefault(kind, {})
                for size, n in h.items():
                    d[size] = d.get(size, 0) + n
        return {k: dict(sorted(v.items())) for k, v in out.items()}

    def close(self):
        for s in self.parts:
            s.ctx.close()


def run_chains(a, dist, dev, X, y, theta_init, measure):
    """One batched-chain run of the benchmark workload on this rank's device: `--warmup`
    untimed transitions per chain, then the timed region (every chain completes >= `--steps`
    transitions under the asynchronous schedule; chains that are ahead keep working; a final
    partial transition is not counted). measure: the roofline HIP-event timing and the
    rocprofv3 window markers bracket the timed region. Returns the sampler (context open) and
    the run's record."""
    from auxpm.batched import BatchedAPMEllSSPlusRandDirSliceSampler
    from gpdemo import _native
    prior = dict(a_tau=1., b_tau=1. / a.d ** 0.5, a_sigma=1.1, b_sigma=0.1)
    if a.chains % a.cohorts:
        raise SystemExit('bench.py: --chains must be a multiple of --cohorts')
    smp = Cohorts(lambda C, first: BatchedAPMEllSSPlusRandDirSliceSampler(
        X, y, C, a.n_imp, prior, kernel='ard', epsilon=1e-8, w=1., max_steps_out=0,
        seed=chain_seed(a.seed, dist.rank), device=dev, first_chain=first), a.chains, a.cohorts)
    smp.initialise(theta_init)
    series = [[] for _ in range(a.chains)]  # every transition of each chain (ESS)
    if a.warmup:
        # every chain W transitions, ending on a transition boundary
        wtr, _ = smp.run_async(a.warmup)
        for c in range(a.chains):
            series[c].extend(wtr[c])
    for ctx in smp.ctxs:
        for k in range(_native.PROF_NKINDS):
            ctx.prof_read(k, reset=True)
        if measure:
            # roofline level: one HIP-event pair per Gram, L.U and rank-512 update launch (the
            # in-panel update launches are not bracketed: their events cost ~2 % of the
            # theta-call)
            ctx.prof_enable(1)
    device_sync()  # first torch touch outside the timed region
    mark = (lambda: smp.ctxs[0].prof_marker(1)) if measure else None  # (tools/prof_window.py)
    th0, u0 = smp.n_theta_calls, smp.n_u_calls
    smp.reset_records()
    res = {}

    def body():
        res['traces'], res['done'] = smp.run_async(a.steps, keep_going=True)
    elapsed = timed_region(dist, body, 1, mark)
    done = res['done']
    for c in range(a.chains):
        series[c].extend(res['traces'][c])
    if measure:
        smp.ctxs[0].prof_marker(2)
        for ctx in smp.ctxs:
            ctx.prof_enable(False)
    done = np.where(smp.failed, 0, done)
    local_tr = int(done.sum())
    transitions = dist.sum(local_tr)
    call_ops = list(smp.call_ops)
    rec = {'elapsed': elapsed, 'done': done, 'local_tr': local_tr, 'transitions': transitions,
           'value': transitions / elapsed, 'series': series, 'traces': res['traces'],
           'n_th': (smp.n_theta_calls - th0) / max(1, local_tr),
           'n_u': (smp.n_u_calls - u0) / max(1, local_tr),
           'call_ops': call_ops, 'wall': dict(smp.wall), 'batch_hist': smp.batch_hist(),
           'theta_call_ms_mean': 1e3 * smp.wall['theta_call'] / max(1, len(call_ops))}
    return smp, rec


DUMP_MAX_BYTES = 48 << 20  # of the theta array (the dump stays below 64 MB)


def dump_outputs(dirname, dist, a, run, P):
    """--dump-outputs: what the timed region's call (run_async(--steps, keep_going=True))
    returned on this rank, as float64 .npy files:
      thetas            (chains, K, P)  each chain's theta after each of its first --steps timed
                                        transitions (every live chain completes that many; what
                                        chains that were ahead did beyond them is left out). K =
                                        --steps, or the last K of them where --steps of them
                                        would pass DUMP_MAX_BYTES. A failed chain's rows are NaN.
      transitions_done  (chains,)       completed timed transitions per chain (0: failed)
    Data, start states and every chain's random streams follow from the arguments alone and the
    schedule does not depend on the clock, so two runs with the same arguments write the same
    arrays. With --gpus N > 1 every rank writes its own chains as <name>_rank<r>.npy."""
    os.makedirs(dirname, exist_ok=True)
    keep = min(a.steps, max(1, DUMP_MAX_BYTES // (8 * a.chains * P)))
    first = a.steps - keep
    th = np.full((a.chains, keep, P), np.nan)
    for c in range(a.chains):
        if run['done'][c] >= a.steps:
            th[c] = np.array(run['traces'][c][first:a.steps])
    suffix = '' if dist.world == 1 else '_rank{0}'.format(dist.rank)
    np.save(os.path.join(dirname, 'thetas' + suffix + '.npy'), th)
    np.save(os.path.join(dirname, 'transitions_done' + suffix + '.npy'),
            np.asarray(run['done'], dtype=np.float64))


def main():
    a = parse()
    dist = Dist()
    if a.gpus != dist.world:
        raise SystemExit('bench.py: --gpus {0} but WORLD_SIZE={1}; launch N>1 as `python -m '
                         'torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr '
                         '127.0.0.1 --master-port P bench.py --gpus N`'.format(a.gpus, dist.world))
    from gpdemo import _native
    from gpdemo.utils import synthetic_gp_data

    dev = rank_device(dist)
    _SYNC_DEVICE[0] = dev
    X, y = synthetic_gp_data(a.n, a.d, a.seed)
    P = a.d + 1
    # headline run: the chains start from the long-chain record's stationary states (the regime
    # a whole chain is made of); where no record fits the workload, from prior draws
    th_stat, stat_src = stationary_states(a, P)
    smp, run = run_chains(a, dist, dev, X, y, th_stat, measure=True)
    elapsed, done, local_tr = run['elapsed'], run['done'], run['local_tr']
    transitions, value = run['transitions'], run['value']
    n_th, n_u, call_ops, wall = run['n_th'], run['n_u'], run['call_ops'], run['wall']
    series = run['series']
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, dist, a, run, P)

    prof = {}
    for k, name in ((_native.PROF_GRAM, 'gram'), (_native.PROF_CHOL_UPDATE_OUTER, 'chol_update'),
                    (_native.PROF_UGEMM, 'ugemm'),
                    (_native.PROF_CHOL_UPDATE32_OUTER, 'chol_update32'),
                    (_native.PROF_POST32_OUTER, 'post32')):
        prof[name] = tuple(np.sum([ctx.prof_read(k, reset=False) for ctx in smp.ctxs], axis=0))
    for ctx in smp.ctxs:
        ctx.prof_read(0, reset=True)
    n_rerun, n_refine, n_df_timeouts, n_trsv_timeouts, n_post64 = np.sum(
        [device_counters(ctx) for ctx in smp.ctxs], axis=0)

    def mfma_roofline(name, kernel, peak, shorts, kind):
        ms, cnt, flops = prof[name]
        if not cnt:
            return None
        avg_s = ms * 1e-3 / cnt
        achieved = (flops / cnt) / avg_s / 1e12
        tr, src = pmc_traffic(*shorts)
        out = {'kernel': kernel, 'bound': 'mfma', 'achieved': achieved, 'peak': peak,
               'unit': 'TFLOP/s', 'frac': achieved / peak, 'traffic': tr,
               'traffic_unit': 'HBM bytes per launch', 'traffic_source': src,
               'launches': cnt, 'avg_launch_us': avg_s * 1e6,
               'algorithmic_flops_per_launch': flops / cnt,
               'share_of_step_time': (ms * 1e-3) / elapsed}
        mf = pmc_mfma(kind, *shorts)
        if mf:
            out['mfma_busy'] = dict(mf, counter_over_algorithmic_flops=mf[
                'counter_flops_per_launch'] / (flops / cnt))
        return out

    upd64 = mfma_roofline('chol_update', 'k_chol_update_t128 (f64 MFMA rank-512 trailing updates '
                          'of the fp64 factorisations: chol(K), the single-launch SYRK and the '
                          'chol of I + L_K^T W L_K)', PEAK_F64_MFMA_TFLOPS,
                          ('k_chol_update_t128',), 'f64')
    upd32 = mfma_roofline('chol_update32', 'k_chol_update32_q256 + k_chol_update32_t128 '
                          '(rank-512 trailing updates of the Newton factorisation of B, fp16x3: '
                          'operands as fp16 hi/lo planes written by the panel kernels, 3 '
                          'v_mfma_f32_16x16x32_f16 per block, fp32 accumulation; the far part on '
                          '256x256 quad tiles, the next panel\'s columns on 128x128 super-tiles; '
                          'achieved in fp32-equivalent flops against the fp16 peak / 3)',
                          PEAK_F16X3_TFLOPS,
                          ('k_chol_update32_q256<0>', 'k_chol_update32_q256',
                           'k_chol_update32_t128<true, 2>', 'k_chol_update32_t128<true, 0>',
                           'k_chol_update32_t128<false, 0>'),
                          'f16x3')
    # the posterior factor's fp32 bottom block: the same kernel under its own instantiation name
    # (ROLE = 1, chol32.hip), so its counter figures are its own
    post32 = mfma_roofline('post32', 'k_chol_update32_q256<1> (fp16x3 operand planes, 256x256 '
                           'quad tiles; k_chol_update32_t128<*, 1> for batches outside fp16\'s '
                           'range) on the posterior factor\'s bottom block (L_K J) L\'^-T, second '
                           'stream; postcov.hip',
                           PEAK_F16X3_TFLOPS,
                           ('k_chol_update32_q256<1>', 'k_chol_update32_t128<true, 1>',
                            'k_chol_update32_t128<false, 1>'),
                           'f16x3')
    # `roofline` is the kernel with the larger share of the step; the other one rides along
    cands = [r for r in (upd64, upd32) if r is not None]
    roofline = max(cands, key=lambda r: r['share_of_step_time'])
    extra = {}
    if post32 is not None:
        extra['roofline_post32'] = post32
    for r, key in ((upd64, 'roofline_update_f64'), (upd32, 'roofline_update_f32')):
        if r is not None and r is not roofline:
            extra[key] = r
    gms, gcnt, gbytes = prof['gram']
    if gcnt:
        ach = gbytes / (gms * 1e-3) / 1e12
        tr, src = pmc_traffic('k_gram_mfma', 'k_gram')
        # the compute side: pairs per launch from the algorithmic bytes (8 (N D + N (N+1) / 2)
        # per chain); the direct form (k_gram, the default) spends a subtract and an fma, 3 fp64
        # flops, per pair and feature on the VALU
        per_chain = 8.0 * (a.n * a.d + 0.5 * a.n * (a.n + 1))
        pairs = (gbytes / gcnt) / per_chain * 0.5 * a.n * (a.n + 1)
        dist_tf = 3.0 * a.d * pairs / (gms * 1e-3 / gcnt) / 1e12
        extra['roofline_gram'] = {'bound': 'hbm', 'achieved': ach, 'peak': PEAK_HBM_TBS,
                                  'unit': 'TB/s', 'frac': ach / PEAK_HBM_TBS, 'traffic': tr,
                                  'traffic_source': src,
                                  'launches': gcnt, 'avg_launch_us': gms * 1e3 / gcnt,
                                  'algorithmic_bytes_per_launch': gbytes / gcnt,
                                  'compute': {'distance_tflops': dist_tf,
                                              'frac_f64_peak': dist_tf / PEAK_F64_MFMA_TFLOPS,
                                              'note': 'direct form sum_k (z_ik - z_jk)^2 on '
                                                      'the fp64 VALU (3 D flops per pair; the '
                                                      'MI355X fp64 vector peak is 78.6 TFLOP/s) '
                                                      'plus one fp64 exp per pair; a GEMM form '
                                                      'on the f64 MFMA was measured and declined '
                                                      '(DESIGN.md §5)'}}
    ums, ucnt, uflops = prof['ugemm']
    if ucnt:
        ach = uflops / (ums * 1e-3) / 1e12
        lu_names = ('k_ugemm<1>', 'k_ugemm<2>', 'k_ugemm')  # (round-3 name: untemplated)
        tr, src = pmc_traffic(*lu_names)
        extra['roofline_lu'] = {'bound': 'mfma', 'achieved': ach, 'peak': PEAK_F32_MFMA_TFLOPS,
                                'unit': 'TFLOP/s', 'frac': ach / PEAK_F32_MFMA_TFLOPS,
                                'traffic': tr, 'traffic_source': src, 'launches': ucnt,
                                'avg_launch_us': ums * 1e3 / ucnt,
                                'algorithmic_flops_per_launch': uflops / ucnt}
        mf = pmc_mfma('f32', *lu_names)
        if mf:
            extra['roofline_lu']['mfma_busy'] = mf

    # ESS (--full): extend the same chains (untimed) until each has >= ess-min transitions after
    # the burn-in, then ESS per transition x the timed transitions/s (ess_block)
    ess = {'ess_per_sec': None, 'ess_mean_per_sec': None, 'rhat': None, 'sample': None}
    if a.full:
        burn = max(a.ess_burn, a.warmup)
        need = np.array([0 if smp.failed[c] else max(0, burn + a.ess_min - len(series[c]))
                         for c in range(a.chains)], dtype=np.int64)
        t_ext = time.perf_counter()
        if need.max() > 0:
            etr, _ = smp.run_async(need)
            for c in range(a.chains):
                series[c].extend(etr[c])
        t_ext = time.perf_counter() - t_ext
        failed_mask = smp.failed
        ess = ess_block(dist, types.SimpleNamespace(n_chains=a.chains, failed=failed_mask),
                        series, done, burn, elapsed, P)
        ess['sample']['untimed_extension_s_rank0'] = t_ext
        ess["sample"]["timed_transitions_per_chain_min"] = int(-dist.max(
            -(done[~failed_mask].min() if (~failed_mask).any() else 0)))
        ess['sample']['timed_transitions_per_chain_max'] = int(dist.max(done.max()))
    failed_mask = smp.failed
    failed = int(dist.sum(int(failed_mask.sum())))
    local_failed = int(failed_mask.sum())
    smp.close()  # frees the chains' workspaces before the next context

    # the same workload from prior draws (the reference notebooks' chain start,
    # E-SS+RD-SS.ipynb:198-201): its first transitions need ~4 Newton iterations per theta-call
    # against 7-8 at stationarity, so it runs faster than the chains a long run is made of
    prior_init = None
    if a.full and th_stat is not None:
        smp2, run2 = run_chains(a, dist, dev, X, y, None, measure=False)
        prior_init = {'value': run2['value'], 'transitions_timed': int(run2['transitions']),
                      'ms_per_step': 1e3 * run2['elapsed'] / a.steps,
                      'theta_calls_per_transition': run2['n_th'],
                      'u_calls_per_transition': run2['n_u'],
                      'theta_call_ms_mean': run2['theta_call_ms_mean'],
                      'cubic_ops_per_theta_call_mean_of_batch_max':
                          float(np.mean([m for m, _ in run2['call_ops']]))
                          if run2['call_ops'] else None,
                      'failed_chains': int(dist.sum(int(smp2.failed.sum())))}
        smp2.close()

    cpu, first, parity = None, None, None
    if a.full:
        sys.path.insert(0, os.path.join(REPO, 'oracle'))
        thetas_par, fix_rows, U1, U2 = parity_inputs(a.n, a.d, a.n_imp)
        if a.cpu_baseline and dist.rank == 0 and dist.world == 1:
            # (N = 1 only, as the bench contract asks; rank 0 alone: a failure here must not
            # strand the others in the parity check)
            try:
                cpu, first = cpu_baseline(X, y, a.n_imp, thetas_par[0], n_th, n_u, a.cpu_budget,
                                          U1, U2)
                cpu['gpu_over_cpu_per_chain'] = (value / (a.chains * dist.world)) / cpu['value']
            except Exception as e:  # noqa: BLE001
                cpu, first = {'error': repr(e)}, None
        if a.parity:
            parity = parity_check(dist, X, y, a, thetas_par, fix_rows, U1, U2, first)

    # per-rank record: device, chains, transitions, elapsed, failures and the device counters of
    # the timed run (8 distinct devices, even load, no silent spin exits)
    mine = np.array([float(dist.rank), float(dev), float(a.chains), float(local_tr),
                     float(elapsed), float(local_failed), n_rerun, n_df_timeouts,
                     n_trsv_timeouts, n_post64])
    ranks = [{'rank': int(r[0]), 'device': int(r[1]), 'chains': int(r[2]),
              'transitions': int(r[3]), 'elapsed_s': r[4], 'failed_chains': int(r[5]),
              'transitions_per_s': r[3] / r[4], 'newton_fp64_reruns': int(r[6]),
              'dataflow_spin_timeouts': int(r[7]), 'trsv_spin_timeouts': int(r[8]),
              'posterior_bottom_fp64_reruns': int(r[9])} for r in dist.all_gather(mine)]

    stationary = th_stat is not None
    line = {
        'metric': METRIC, 'value': value, 'unit': 'transitions/s (all chains, all GPUs)',
        'n_gpus': dist.world, 'steps': a.steps, 'warmup': a.warmup, 'full': a.full,
        'ms_per_step': 1e3 * elapsed / a.steps,
        'ms_per_step_note': 'timed wall time / --steps; under the asynchronous schedule every '
                            'chain completes >= --steps transitions (chains ahead keep working), '
                            'so this is neither a lockstep step time nor a per-transition time: '
                            'see ms_per_transition_per_chain',
        'ms_per_transition_per_chain': 1e3 * elapsed * a.chains * dist.world / max(1, transitions),
        'higher_is_better': True, 'scaling': 'weak',
        'vs_baseline': None, 'dtype': 'mixed f64/f32',
        'dtype_detail': 'theta-path Gram, chol(K) and the posterior-covariance factor fp64 on f64 '
                        'MFMA; Newton matrix B factored in fp32 (trailing updates fp16x3: fp16 '
                        'hi/lo operand splits, fp32 accumulation; panels fp32) with fp64 iterative '
                        'refinement of each solve (mode = fp64 Newton mode to ~1e-12); '
                        'importance-sampling L.U fp32 on f32 MFMA; probit/LME epilogue fp32->fp64',
        'data': 'synthetic (X~N(0,1) normalised, y=sign of a GP prior draw; seed {0})'.format(a.seed),
        'config': {'workload': 'APM E-SS(u) + RD-SS(theta), ARD-SE probit GP classification, '
                               'ApproxPosteriorIS estimator, N=4096 D=32 N_imp=256 (BASELINE.json '
                               'configs[2]; 64 chains per GPU = the per-GPU share of configs[3])',
                   'n_data': a.n, 'n_features': a.d, 'n_imp': a.n_imp, 'n_theta': P,
                   'chains_per_gpu': a.chains, 'global_batch': a.chains * dist.world,
                   'parallelism': 'dp{0} (independent chains per GPU, no collective)'
                   .format(dist.world),
                   'cohorts_per_gpu': a.cohorts,
                   'chain_start': ('stationary: the long-chain record\'s chain states ({0}), '
                                   'fresh u, then --warmup transitions'.format(stat_src)
                                   if stationary else
                                   'prior draws (E-SS+RD-SS.ipynb:198-201): {0}'.format(stat_src))},
        'value_prior_init': prior_init,
        'ess_per_sec': ess['ess_per_sec'], 'ess_mean_per_sec': ess['ess_mean_per_sec'],
        'ess_per_sec_source': ('in-run sample of this run\'s chains (ess_sample)' if a.full else
                               'none: the in-run sample is taken with --full'),
        'ess_per_sec_in_run': ess['ess_per_sec'], 'ess_mean_per_sec_in_run': ess['ess_mean_per_sec'],
        'rhat': ess['rhat'], 'ess_sample': ess['sample'],
        'parity': parity,
        'schedule': a.schedule, 'transitions_timed': int(transitions),
        'theta_calls_per_transition': n_th, 'u_calls_per_transition': n_u,
        'theta_call_ms_mean': run['theta_call_ms_mean'],
        'failed_chains': failed,
        'newton_refinement_steps': int(dist.sum(n_refine)),
        'newton_fp64_reruns': int(dist.sum(n_rerun)),
        'posterior_bottom_fp64_reruns': int(dist.sum(n_post64)),
        'newton_dataflow_spin_timeouts': int(dist.sum(n_df_timeouts)),
        'newton_trsv_spin_timeouts': int(dist.sum(n_trsv_timeouts)),
        'cubic_ops_per_theta_call': {
            'mean_of_batch_max': float(np.mean([m for m, _ in call_ops])) if call_ops else None,
            'mean_of_batch_mean': float(np.mean([v for _, v in call_ops])) if call_ops else None,
            'note': 'IS: Newton iterations + 3 (estimators.py:217); a batched call lasts as long '
                    'as its slowest chain'},
        'wall_split_s': dict(wall, host_sampler=elapsed - sum(wall.values())),
        'calls_by_batch_size': run['batch_hist'],
        'ranks': ranks,
        'roofline': roofline, 'cpu_baseline': cpu,
    }
    line.update(extra)
    # the PMC numbers (traffic, mfma_busy) come from a committed counter pass: of this build?
    line['pmc_provenance'] = pmc_provenance()
    line['ess_long_chain'] = lr = ess_long_record(value, a)
    if lr is not None and stationary:
        # the headline ESS/s: the long-chain record's ESS per transition (its chains have run
        # 22 000 transitions; this run's ~150-transition series cannot see the slow modes) x
        # THIS run's driver-timed stationary transitions/s
        line['ess_per_sec'] = lr['ess_per_sec_estimate']
        line['ess_mean_per_sec'] = lr['ess_mean_per_sec_estimate']
        line['ess_per_sec_source'] = (
            'long-chain record {0}: ESS per transition (min over theta components, {1:.5f}) x '
            'this run\'s driver-timed transitions/s from the record\'s stationary states '
            '(value, {2:.1f}); R-hat max {3:.3f} ({4}); the in-run figure is ess_per_sec_in_run'
            .format(lr['source'], lr['ess_per_transition_min_component'], value, lr['rhat_max'],
                    'converged' if lr['converged_rhat_below_1p1'] else
                    'NOT converged: R-hat > 1.1'))
    # the paper's efficiency column N_eff / N_cub.op (Analyse results.ipynb: effectiveSize over
    # the run's n_cubic_ops / 1000, n_cubic_ops counted as estimators.py:81,217,322 - an IS
    # theta-call costs its Newton iterations + 3, a cached u-call none): ESS per transition ÷
    # cubic ops per transition x 1000, from the long-chain record's ESS per transition and this
    # run's theta-calls per transition x cubic ops per theta-call (per chain)
    cops_call = line['cubic_ops_per_theta_call']['mean_of_batch_mean']
    if lr is not None and cops_call and n_th:
        cop_tr = n_th * cops_call
        eptm = lr.get('ess_per_transition_mean_component')
        line['ess_per_kcop'] = {
            'min_component': 1e3 * lr['ess_per_transition_min_component'] / cop_tr,
            'mean_component': 1e3 * eptm / cop_tr if eptm is not None else None,
            'cubic_ops_per_transition': cop_tr,
            'source': 'long-chain record {0} (ESS per transition; R-hat max {1:.3f}) / (this '
                      'run\'s theta_calls_per_transition {2:.3f} x cubic_ops_per_theta_call '
                      'mean_of_batch_mean {3:.3f}) x 1000; Analyse results.ipynb '
                      'N_eff/N_cub.op'.format(lr['source'], lr['rhat_max'], n_th, cops_call)}
    if dist.rank == 0:
        print(json.dumps(line), flush=True)
    ok = parity is None or parity['pass']
    dist.close()
    del _native
    if not ok:
        if dist.rank == 0:
            print('bench.py: PARITY FAILED; parity block: ' + json.dumps(parity), file=sys.stderr,
                  flush=True)
        sys.exit(3)


if __name__ == '__main__':
    main()
