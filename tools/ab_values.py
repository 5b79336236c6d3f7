"""Values of one library build for a bitwise A/B against another (development tool).

Full size: the 64-chain stationary theta-call + cached u-call at N=4096 (and a ragged N=1100
case), the outputs and slot factors saved to an npz.

    APM_LIB=path/to/libapm.so python tools/ab_values.py out.npz

Small shapes (`--small`): every host path of the library at the sizes where its schedule
changes - N = 64 and 65 (nb = 1, 2: the 64x64 update and identity-SYRK path against the smallest
128x128 / single-launch SYRK path), N = 1089 with d = 5 ARD (nb = 18: three outer panels, a
partial Gram copy, the Newton lookahead with far updates, explicit-inverse panels), a Matern
5/2 ARD context at N = 200, and two isotropic kinds whose features need a second LDS chunk of the
pair-distance tile (csrc/pair_tile.h): SE at N = 130, d = 40 (a second chunk of 8 features) and
Matern 3/2 at N = 129, d = 33 (the two-pass gradient, a second chunk of one feature, a last tile
of one row), and the N = 65 shape once more with 9 chains (n65x9: its three thetas on 9 slots and
9 distinct U buffers), whose 2 x 1 x 9 = 18 work items run the u-path's fp32 kernels in their
XCD-remapped order (8 chains and more; 18 is no multiple of 8). One case is one shape under one
setting of the environment knobs;
run each in a process of its own (the knobs are read when a context is created):

    python tools/ab_values.py --list-small
    APM_LIB=... python tools/ab_values.py --small n1089:APM_POST32_Q=0 out_dir/

The default setting of a shape runs every call (IS theta-call + u-call + slot read, apm_is_loo and
apm_is_loo_psis with the log ratios on that u-call's samples, PriorMC, Laplace, apm_theta_eval_K, apm_predict with one and three row tiles of test inputs,
apm_laplace_grad, apm_ep_eval / apm_ep_predict / apm_ep_grad, the EST_IS_EP theta-call,
apm_is_predict with both proposals and one and two blocks of test inputs, apm_u_eval_diag,
apm_is_spread, apm_laplace and apm_ep with their covariances); a knob setting repeats the IS call,
which is what the knobs reach, and APM_WIDE_Q=0 (every slot wide: the u-path's f64 kernels) the two
LOO calls as well. n65x9 runs the IS call and the two LOO calls, under those two settings. After every call the launch counts of all APM_PROF_* kinds (profiling
level 2) are saved beside the arrays.

    python tools/ab_values.py --compare a.npz b.npz      (or two directories of npz files)
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'auxiliary-pm-mcmc_amd'))
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, os.path.join(REPO, 'tests'))  # grad_restatement.make_case, edge_cases.SEEDS

# name -> (n, d, kernel kind name, data seed); 65 and 1089 take tests/edge_cases.py's seeds
SMALL_SHAPES = {'n64': (64, 4, 'KERNEL_ARD', 3064), 'n65': (65, 4, 'KERNEL_ARD', None),
                'n1089': (1089, 5, 'KERNEL_ARD', None), 'm200': (200, 4, 'KERNEL_M52_ARD', 5200),
                'iso130': (130, 40, 'KERNEL_ISO', 3170), 'm129': (129, 33, 'KERNEL_M32_ISO', 5162),
                'n65x9': (65, 4, 'KERNEL_ARD', None)}
REMAP = 'n65x9'  # n65's thetas three times over: 9 chains
# the knobs that reach a rare host path: fp64 Newton; fp32 operands; fp64 rerun, then chol(K)
# again on the main stream; the fp64 bottom block with its gap; attach / rewrite of fp64 slot
# factors; the reference-route check of every chain (the value tests/test_gpu_configs.py uses)
SMALL_KNOBS = ('', 'APM_MIXED=0', 'APM_H3=0', 'APM_REFINE_TOL=0', 'APM_POST32_Q=0',
               'APM_WIDE_Q=0', 'APM_ICM_Q=1')
LOO_KNOBS = ('', 'APM_WIDE_Q=0')  # the settings that also run apm_is_loo and apm_is_loo_psis
S_IMP = 16


def small_cases():
    return ['{0}:{1}'.format(s, k) if k else s for s in SMALL_SHAPES for k in SMALL_KNOBS
            if s != REMAP or k in LOO_KNOBS]


def run(path):
    from gpdemo import _native
    from gpdemo import utils
    out = {}
    X, y = utils.synthetic_gp_data(4096, 32, 20151009)
    th = np.load(os.path.join(REPO, 'tests', 'golden', 'stationary_thetas.npy')).astype(np.float64)
    cases = [('stat', X, y, th, 256, 64)]
    X2, y2 = utils.synthetic_gp_data(1100, 5, 4242, 'ard')
    rng = np.random.RandomState(7)
    th2 = np.array([np.r_[t0, rng.normal(scale=0.3, size=5) + 0.5 * np.log(5)]
                    for t0 in (0.0, 2.0, 4.0)])
    cases.append(('n1100', X2, y2, th2, 32, 3))
    for name, Xc, yc, thc, s, B in cases:
        ctx = _native.Context(Xc, yc, _native.KERNEL_ARD, 1e-8, s, max_batch=B, n_slots=B,
                              n_ubufs=B)
        idx = np.arange(B)
        ctx.u_normal(idx, np.full(B, 7), idx)
        v1, st, nops = ctx.theta_eval(_native.EST_IS, thc, idx, idx)
        v2, st2 = ctx.u_eval(idx, idx)
        out[name + '_v1'], out[name + '_v2'], out[name + '_st'] = v1, v2, st
        for b in range(min(B, 4)):
            L, f, g, c = ctx.slot_read(b)
            out['{0}_L{1}'.format(name, b)] = L.astype(np.float32)
            out['{0}_f{1}'.format(name, b)] = f
        ctx.close()
    np.savez(path, **out)


def run_small(case, outdir):
    shape, _, knob = case.partition(':')
    if knob:
        key, _, val = knob.partition('=')
        os.environ[key] = val  # (before the first context: read by apm_create)
    from gpdemo import _native
    import edge_cases
    import grad_restatement as gr
    n, d, kind_name, seed = SMALL_SHAPES[shape]
    kind = getattr(_native, kind_name)
    c = gr.make_case(n, d, 'iso' if kind_name.endswith('_ISO') else 'ard',
                     edge_cases.SEEDS[n] if seed is None else seed)
    X, y, th = c['X'], c['y'], c['thetas']
    if shape == REMAP:
        th = np.tile(th, (3, 1))
    B = th.shape[0]
    idx = np.arange(B)
    out = {}

    def context():
        ctx = _native.Context(X, y, kind, 1e-8, S_IMP, max_batch=B, n_slots=B, n_ubufs=B)
        ctx.prof_enable(2)
        ctx.u_normal(idx, np.full(B, 7), idx)  # (one counter per buffer: the chains differ)
        return ctx

    def launches(ctx, call):
        # (a reset of one kernel kind drops the records of all: read everything first)
        out[call + '_launches'] = np.array(
            [ctx.prof_read(k)[1] for k in range(_native.PROF_NKINDS)], dtype=np.int64)
        for k in range(_native.PROF_NKINDS):
            ctx.prof_read(k, reset=True)

    def slots(ctx, call):
        for b in range(B):
            L, f, g, cst = ctx.slot_read(b)
            out['{0}_L{1}'.format(call, b)], out['{0}_f{1}'.format(call, b)] = L, f
            out['{0}_g{1}'.format(call, b)], out['{0}_c{1}'.format(call, b)] = g, np.array(cst)

    ctx = context()
    v1, st, nops = ctx.theta_eval(_native.EST_IS, th, idx, idx)
    v2, st2 = ctx.u_eval(idx, idx)
    out.update(is_v1=v1, is_st=st, is_nops=nops, is_v2=v2, is_st2=st2, is_guard=ctx.guard_read(B))
    slots(ctx, 'is')
    launches(ctx, 'is')
    if knob in LOO_KNOBS:
        for k, a in zip(('logf', 'loo', 'lpd', 'essloo', 'gauss', 'ess', 'st'),
                        ctx.is_loo(idx, idx)):
            out['loo_' + k] = a
        launches(ctx, 'loo')
        for k, a in zip(('logf', 'loo', 'khat', 'khatw', 'logratio', 'st'),
                        ctx.is_loo_psis(idx, idx, want_logratio=True)):
            out['psis_' + k] = a
        launches(ctx, 'psis')
    ctx.close()
    if not knob and shape != REMAP:
        ctx = context()
        v, st, nops = ctx.theta_eval(_native.EST_PRIORMC, th, idx, idx)
        out.update(pmc_v=v, pmc_st=st, pmc_nops=nops)
        slots(ctx, 'pmc')
        launches(ctx, 'pmc')
        v, st, nops = ctx.theta_eval(_native.EST_LAPLACE, th)
        out.update(lap_v=v, lap_st=st, lap_nops=nops)
        launches(ctx, 'lap')
        for m in (40, 150):  # one and three row tiles of test inputs
            Xs = edge_cases.predict_inputs(c, m, 1000.0)
            for k, a in zip(('mean', 'var', 'prob', 'st', 'nit'), ctx.predict(th, Xs)):
                out['pred{0}_{1}'.format(m, k)] = a
            launches(ctx, 'pred{0}'.format(m))
        for k, a in zip(('lml', 'grad', 'st', 'nit'), ctx.laplace_grad(th)):
            out['grad_' + k] = a
        launches(ctx, 'grad')
        Xs = edge_cases.predict_inputs(c, 40, 1000.0)
        for call, names, fn in (
                ('ep', ('logz', 'mu', 'var', 'tau', 'nu', 'st', 'nsw'), lambda: ctx.ep(th)),
                ('eppred', ('mean', 'var', 'prob', 'st', 'nsw'), lambda: ctx.ep_predict(th, Xs)),
                ('epgrad', ('logz', 'grad', 'st', 'nsw'), lambda: ctx.ep_grad(th))):
            for k, a in zip(names, fn()):
                out['{0}_{1}'.format(call, k)] = a
            launches(ctx, call)
        ctx.close()
        ctx = context()
        v1, st, nops = ctx.theta_eval(_native.EST_IS_EP, th, idx, idx)
        v2, st2 = ctx.u_eval(idx, idx)
        out.update(isep_v1=v1, isep_st=st, isep_nops=nops, isep_v2=v2, isep_st2=st2)
        slots(ctx, 'isep')
        launches(ctx, 'isep')
        # one block of test inputs and two (n1089: one, and two replicates, to stay short)
        big = n > 1024
        for est, nm in ((_native.EST_IS, 'ispred'), (_native.EST_IS_EP, 'iseppred')):
            for m in (40,) if big else (40, ctx.padded_n + 1):
                call = '{0}{1}'.format(nm, m)
                res = ctx.is_predict(est, th, idx, idx, edge_cases.predict_inputs(c, m, 1000.0))
                for k, a in zip(('logf', 'prob', 'mean', 'var', 'ess', 'st', 'nops'), res):
                    out['{0}_{1}'.format(call, k)] = a
                launches(ctx, call)
        for k, a in zip(('logf', 'ess', 'wmax', 'st'), ctx.u_eval_diag(idx, idx, 4)):
            out['diag_' + k] = a
        launches(ctx, 'diag')
        res = ctx.is_spread(idx, idx, np.full(B, 11, dtype=np.uint64),
                            np.arange(B, dtype=np.uint64), 2 if big else 3, 8)
        for k, a in zip(('logf', 'ess', 'wmax', 'st'), res):
            out['spread_' + k] = a
        launches(ctx, 'spread')
        ctx.close()
        # a host K: the device's own Gram at the first theta (compared as well)
        K = np.empty((n, n))
        _native.gram(kind, K, X, th[0], 1e-8)
        out['gram_K'] = K
        ctx = _native.Context(None, y, _native.KERNEL_PRECOMPUTED, 1e-8, S_IMP, max_batch=1,
                              n_slots=1, n_ubufs=1)
        ctx.prof_enable(2)
        ctx.u_normal([0], [7], [0])
        for est, nm in ((_native.EST_IS, 'kis'), (_native.EST_PRIORMC, 'kpmc'),
                        (_native.EST_LAPLACE, 'klap')):
            v, st, nops = ctx.theta_eval_K(est, K, 0, 0)
            out.update({nm + '_v': v, nm + '_st': st, nm + '_nops': nops})
            launches(ctx, nm)
        L, f, g, cst = ctx.slot_read(0)
        out.update(kpmc_L=L, kpmc_f=f)
        ctx.close()
        f, C, lml, nit, st = _native.laplace(K, y, True, True, 1e-4, 1000)
        out.update(lapcov_f=f, lapcov_C=C, lapcov_lml=np.array(lml), lapcov_nit=np.array(nit),
                   lapcov_st=np.array(st))
        for k, a in zip(('mu', 'var', 'tau', 'nu', 'C', 'logz', 'nsw', 'st'),
                        _native.ep(K, y, True, 0.8, 1e-8, 100)):
            out['epcov_' + k] = np.array(a)
    os.makedirs(outdir, exist_ok=True)
    np.savez(os.path.join(outdir, case.replace(':', '__').replace('=', '_') + '.npz'), **out)
    print('{0}: {1} arrays'.format(case, len(out)))


def compare(a, b):
    """Bitwise (NaNs of equal bit pattern are equal); returns the number of differing arrays."""
    if os.path.isdir(a):
        files = sorted(f for f in os.listdir(a) if f.endswith('.npz'))
        bad = total = counters = 0
        for f in files:
            za, zb = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
            assert sorted(za.files) == sorted(zb.files), f
            for k in za.files:
                total += 1
                counters += k.endswith('_launches')
                xa, xb = np.ascontiguousarray(za[k]), np.ascontiguousarray(zb[k])
                if xa.shape != xb.shape or xa.tobytes() != xb.tobytes():
                    bad += 1
                    print('DIFFERENT {0} {1}'.format(f, k))
        print('{0} files, {1} arrays of which {2} launch-count vectors: {3}'.format(
            len(files), total, counters, 'bitwise identical' if not bad else
            '{0} DIFFERENT'.format(bad)))
        return bad
    za, zb = np.load(a), np.load(b)
    same = True
    for k in za.files:
        d = np.abs(za[k].astype(np.float64) - zb[k].astype(np.float64)).max()
        same &= d == 0
        print('{0:12s} max |a - b| = {1:.3e}'.format(k, d))
    print('bitwise identical' if same else 'DIFFERENT')
    return 0 if same else 1


if __name__ == '__main__':
    if sys.argv[1] == '--compare':
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    elif sys.argv[1] == '--list-small':
        print('\n'.join(small_cases()))
    elif sys.argv[1] == '--small':
        run_small(sys.argv[2], sys.argv[3])
    else:
        run(sys.argv[1])
