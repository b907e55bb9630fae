"""The block estimators of a sharded DMC population: the walker record carries
the per-walker rows of every estimator slot (`DmcEnsemble.set_record_rows`),
`DistributedDmc(..., block_estimators=True)` accepts them and `read_estimator`
hands out the rows summed over the ranks.  One GPU: a world of one, and two
handles driven as two ranks, as in tests/test_gpu_dist.py.

The yardsticks are the NumPy restatements of the single-GPU tests, on the
per-step `(confs, cloning_ref, num_walkers)` of `get_state()`:

* g2(r) and the site statistics, both pure: integers until the one division,
  compared with `array_equal` (tests/test_gpu_pairdist_est.py,
  tests/test_gpu_site_est.py);
* the centre-of-mass diffusion: `tolerance` of tests/_cmdiff_restatement.py,
  g = 4 N^2 L 2^-53 per step and walker, T g per walker after T steps,
  (nw T g, nw 2 max|Y| T g) for a row;
* F(k, tau): `tolerance` of tests/_isf_restatement.py;
* g1(s): 2e-11 sum_s max(1, |g1_s|), the definition's bound of
  tests/test_gpu_obdm_est.py.

A transfer between slots is a permutation pi of the parents: the restatement
of a block in which walkers were moved before step t runs on the recorded
steps with step t's cloning table replaced by pi[cloning_ref].

Record layout with everything set at N = 16 (S(k) 8 modes, density 12 bins, g2
10 bins, F(k, tau) 3 x (2 + 2), site 4 + 9):
pos 16 | drift 16 | label 16 | energy | log-weight | S(k) 24 | density 12 |
g2 10 | centre of mass 1 | F(k, tau) 12 | site 13.
"""
import types
from typing import NamedTuple

import numpy as np
import pytest

from . import _cmdiff_restatement as cm
from . import _dmc_walks as walks
from . import _isf_restatement as isf
from . import _obdm_restatement as obdm
from . import _pairdist_fw_restatement as fw
from . import _site_restatement as sr
from ._dmc_walks import EST, TIME_STEP, WALKS
from ._models import model_dict

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
RATIO = 1
HALF_ZB = sr.half_barrier(RATIO)
RTOL_G1 = 2e-11                 # of tests/test_gpu_obdm_est.py
G2_BINS, PFW = 10, 3
SITE_P, SITE_D = 4, 9
SHIFTS = (0.0, 0.5, 1.25)
G1_STRIDE = 2
KEYS = ('pair_dist', 'cm_diffusion', 'isf', 'obdm', 'site')


class Shape(NamedTuple):
    steps: int
    ktq: tuple                  # (K, T, q) of F(k, tau)


# The walks of the same names.  `wide`: the widest row there is,
# 16 x (62 + 2) = 1024 doubles per walker.
SHAPES = {
    'small': Shape(12, (3, 2, 2)),
    'wide':  Shape(8, (16, 62, 1)),
}


def make_engine(shape):
    import torch
    return walks.engine(WALKS[shape],
                        stream=torch.cuda.current_stream().cuda_stream)


def make_ensemble(eng, shape, **kw):
    return walks.ensemble(eng, WALKS[shape], **kw)


def set_all(d, ktq, pure=True):
    d.set_estimators(**EST)
    d.set_pair_dist_estimator(G2_BINS, pure=pure, pfw=PFW)
    d.set_site_estimator(SITE_P, SITE_D, pure=pure, pfw=PFW)
    d.set_cm_diffusion_estimator(True)
    d.set_isf_estimator(*ktq)
    d.set_obdm_estimator(SHIFTS, G1_STRIDE)


def export(d, first, count):
    """-> (device buffer, records[count, record size] on the host)."""
    import torch
    rec = d.walker_record_size()
    buf = torch.zeros(count * rec, dtype=torch.float64, device='cuda')
    d.export_walkers(first, count, buf.data_ptr())
    d.engine.sync()
    return buf, buf.cpu().numpy().reshape(count, rec)


def cm_per_walker(steps, L):
    """Y_t[s] of tests/_cmdiff_restatement.py for every walker, by the same
    operations (its rows are the sums of these: asserted)."""
    ys, x_prev, y_prev = [], None, None
    rows = np.zeros((len(steps), 2))
    for t, (confs, ref, nw) in enumerate(steps):
        x = confs[:nw].sum(axis=1)
        y = np.zeros(nw)
        if t > 0:
            raw = x - x_prev[ref[:nw]]
            y = y_prev[ref[:nw]] + (raw - L * np.rint(raw / L))
        rows[t] = y.sum(), (y * y).sum()
        ys.append(y)
        x_prev, y_prev = x, y
    assert np.array_equal(rows, cm.cm_diffusion(steps, L)[0])
    return ys


def restate(steps, shape, which=('pair_dist', 'site', 'cm_diffusion', 'isf')):
    """-> dict key: (rows, tolerance or None where they are exact)."""
    n, L, ktq = WALKS[shape].n, float(WALKS[shape].sites), SHAPES[shape].ktq
    nws = [s[2] for s in steps]
    out = {}
    if 'pair_dist' in which:
        out['pair_dist'] = (fw.forward_walk(steps, L, G2_BINS, PFW)[1], None)
    if 'site' in which:
        out['site'] = (sr.forward_walk(steps, L, HALF_ZB, SITE_P, SITE_D,
                                       PFW)[1], None)
    if 'cm_diffusion' in which:
        out['cm_diffusion'] = (cm.cm_diffusion(steps, L)[0],
                               cm.tolerance(steps, n, L))
    if 'isf' in which:
        out['isf'] = (isf.isf_rows(steps, L, *ktq),
                      isf.tolerance(n, ktq[0], ktq[1], nws))
    return out


def check_rows(got, want, where=''):
    for key, (rows, tol) in want.items():
        assert got[key].shape == rows.shape, (where, key)
        if tol is None:
            assert np.array_equal(got[key], rows), (where, key)
            continue
        err = np.abs(got[key] - rows)
        print(where, key, 'max err / tol',
              float((err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all(), (where, key, np.argwhere(err > tol)[:8])


def read_all(d, nts):
    return {'pair_dist': d.read_pair_dist(nts), 'site': d.read_site(nts),
            'cm_diffusion': d.read_cm_diffusion(nts), 'isf': d.read_isf(nts)}


# ---- 1. layout -------------------------------------------------------------

def test_record_layout_follows_the_switch_and_the_slots():
    eng = make_engine('small')
    d = make_ensemble(eng, 'small', external_reduce=True)
    n = 16
    base = 3 * n + 2 + 3 * 8 + 12
    assert not d.record_rows
    set_all(d, (3, 2, 2))
    assert d.walker_record_size() == base
    d.set_record_rows(True)
    assert d.record_rows
    assert d.walker_record_size() == base + 10 + 1 + 3 * 4 + 13
    # mixed g2 / site statistics keep no rows: exactly their segments go
    d.set_pair_dist_estimator(G2_BINS, pure=False)
    assert d.walker_record_size() == base + 1 + 3 * 4 + 13
    d.set_site_estimator(SITE_P, SITE_D, pure=False)
    assert d.walker_record_size() == base + 1 + 3 * 4
    d.set_pair_dist_estimator(G2_BINS, pure=True, pfw=PFW)
    assert d.walker_record_size() == base + 10 + 1 + 3 * 4
    d.set_site_estimator(SITE_P, SITE_D, pure=True, pfw=PFW)
    # g1 adds nothing
    d.set_obdm_estimator(None)
    assert d.walker_record_size() == base + 10 + 1 + 3 * 4 + 13
    d.set_obdm_estimator(SHIFTS, G1_STRIDE)
    assert d.walker_record_size() == base + 10 + 1 + 3 * 4 + 13
    # the switch set before the estimators, and off again
    d.set_cm_diffusion_estimator(False)
    d.set_isf_estimator(0)
    assert d.walker_record_size() == base + 10 + 13
    d.set_isf_estimator(3, 2, 2)
    assert d.walker_record_size() == base + 10 + 3 * 4 + 13
    d.set_record_rows(False)
    assert not d.record_rows and d.walker_record_size() == base
    d.close()
    eng.close()


def test_record_of_ssf_and_density_alone_does_not_change_with_the_switch():
    """Two steps and one estimator step in, so that every field is live."""
    from phd_qmclib_amd.dist import DistributedDmc
    eng = make_engine('small')
    d = make_ensemble(eng, 'small', external_reduce=True)
    d.set_estimators(**dict(EST, dens_pure=True, dens_pfw=PFW))
    dd = DistributedDmc(d, 16, 'cuda', rebalance_every=0)
    d.est_begin_block(4)
    for t in range(3):
        dd.step()
        d.step_estimators(t)
    nw = d.num_walkers()
    off = export(d, 0, nw)[1]
    d.set_record_rows(True)
    on = export(d, 0, nw)[1]
    assert off.shape == (nw, 3 * 16 + 2 + 24 + 12)
    assert off.tobytes() == on.tobytes()
    assert np.abs(off[:, 50:]).max() > 0 and off[:, 32:48].max() == 15
    d.close()
    eng.close()


# ---- 2. pack ---------------------------------------------------------------

def test_pack_reads_the_rows_of_the_last_estimator_step():
    from phd_qmclib_amd.dist import DistributedDmc
    shape = 'small'
    n, L, nts = WALKS[shape].n, WALKS[shape].sites, SHAPES[shape].steps
    K, T, q = SHAPES[shape].ktq
    eng = make_engine(shape)
    d = make_ensemble(eng, shape, external_reduce=True)
    set_all(d, (K, T, q))
    dd = DistributedDmc(d, n, 'cuda', rebalance_every=0,
                        block_estimators=True)
    o_g2 = 3 * n + 2 + 24 + 12
    o_cm, o_isf, o_site = o_g2 + 10, o_g2 + 11, o_g2 + 11 + K * (T + 2)
    assert d.walker_record_size() == o_site + SITE_P + SITE_D
    d.est_begin_block(nts)
    steps, packed = [], {}
    for t in range(nts):
        dd.step()
        d.step_estimators(t)
        steps.append(walks.state_of(d))
        if t in (4, 5):                 # written to rows buffer 0, buffer 1
            recs = export(d, 0, steps[-1][2])[1]
            rows = read_all(d, nts)
            div = float(min(t + 1, PFW))
            got = recs[:, o_g2:o_cm].sum(axis=0) / div
            assert np.array_equal(got, rows['pair_dist'][t]) and got.any()
            got = recs[:, o_site:].sum(axis=0) / div
            assert np.array_equal(got, rows['site'][t]) and got.any()
            got = recs[:, o_isf:o_site].sum(axis=0).reshape(K, T + 2)
            tol = isf.tolerance(n, K, T, [steps[-1][2]])[0]
            assert (np.abs(got - rows['isf'][t]) <= tol).all()
            assert got[:, :2].all() and got[1:].all()
            packed[t] = recs[:, o_cm].copy()
    # the centre-of-mass row of walker s after step t is the Y that its
    # children yield at step t + 1
    ys = cm_per_walker(steps, float(L))
    g = 4.0 * n * n * L * EPS
    for t, seg in packed.items():
        ref = steps[t + 1][1][:steps[t + 1][2]]
        err = np.abs(seg[ref] - ys[t + 1])
        assert len(set(ref)) > 100 and np.abs(ys[t + 1]).min() > 0
        assert (err <= (t + 1) * g).all(), err.max()
    d.close()
    eng.close()


# ---- 3. unpack: the rows follow the walker ---------------------------------

def swapped_run(shape, when, k, isf_only):
    """-> (steps as recorded, pi, device rows)."""
    import torch
    from phd_qmclib_amd.dist import DistributedDmc
    n, maxw = WALKS[shape].n, WALKS[shape].maxw
    nts, ktq = SHAPES[shape].steps, SHAPES[shape].ktq
    eng = make_engine(shape)
    d = make_ensemble(eng, shape, external_reduce=True)
    if isf_only:
        d.set_isf_estimator(*ktq)
    else:
        set_all(d, ktq)
    dd = DistributedDmc(d, n, 'cuda', rebalance_every=0,
                        block_estimators=True)
    assert d.record_rows
    d.est_begin_block(nts)
    steps, perm = [], np.arange(maxw)
    for t in range(nts):
        if t == when:
            nw = d.num_walkers()
            assert nw >= 2 * k
            bx, hx = export(d, nw - 2 * k, k)
            by, hy = export(d, nw - k, k)
            d.import_walkers_at(nw - 2 * k, k, by.data_ptr())
            d.import_walkers_at(nw - k, k, bx.data_ptr())
            assert d.num_walkers() == nw
            assert export(d, nw - 2 * k, k)[1].tobytes() == hy.tobytes()
            assert export(d, nw - k, k)[1].tobytes() == hx.tobytes()
            assert hx.tobytes() != hy.tobytes()
            perm[nw - 2 * k:nw - k] = np.arange(nw - k, nw)
            perm[nw - k:nw] = np.arange(nw - 2 * k, nw - k)
            torch.cuda.synchronize()
        dd.step()
        d.step_estimators(t)
        steps.append(walks.state_of(d))
    rows = {'isf': d.read_isf(nts)} if isf_only else read_all(d, nts)
    d.close()
    eng.close()
    return steps, perm, rows


@pytest.mark.parametrize('shape,when,k', [
    ('small', 5, 37), ('small', 6, 37),       # odd and even: both row buffers
    # (64 walkers: two ranges of 37 do not fit; 21 is odd as well)
    ('wide', 5, 21)])
def test_imported_rows_follow_the_walker_not_the_slot(shape, when, k):
    isf_only = shape == 'wide'
    which = ('isf',) if isf_only else ('pair_dist', 'site', 'cm_diffusion',
                                       'isf')
    steps, perm, rows = swapped_run(shape, when, k, isf_only)
    moved = list(steps)
    confs, ref, nw = steps[when]
    moved[when] = (confs, perm[ref], nw)
    want = restate(moved, shape, which)
    check_rows(rows, want, f'{shape} {when}')
    # rows that had stayed with the slots would be far off
    stay = restate(steps, shape, which)
    for key in which:
        far, tol = stay[key][0] - want[key][0], want[key][1]
        if tol is None:
            assert far.any(), key
        else:
            assert (np.abs(far) > 100 * tol).any(), key


# ---- 4. two shards, one population -----------------------------------------

def test_two_shards_sum_to_the_union():
    """Set up as test_gpu_dist.py::test_two_shards_one_population: 90 and 30
    walkers, one target of 120 and one E_ref; 30 tail walkers go from a to b
    before step 5, their rows with them."""
    import torch
    from phd_qmclib_amd.dist import _wrap_f64
    from phd_qmclib_amd.engine import DmcEnsemble
    from phd_qmclib_amd.qmc_base import dmc_est
    shape = 'small'
    n, nts, ktq = WALKS[shape].n, SHAPES[shape].steps, SHAPES[shape].ktq
    L, cap, k = float(WALKS[shape].sites), 160, 30
    eng = make_engine(shape)
    pos = [L * np.random.RandomState(s).random_sample((w, n))
           for s, w in ((21, 90), (22, 30))]
    e_ref = []
    for p in pos:
        h = DmcEnsemble(eng, TIME_STEP, cap, len(p), 0.5, rng_seed=21,
                        external_reduce=True)
        h.set_state(p)
        e_ref.append(h.get_scalars()[2])
        h.close()
    ref_energy = (90 * e_ref[0] + 30 * e_ref[1]) / 120
    shards = []
    for slot0, p in zip((0, cap), pos):
        h = DmcEnsemble(eng, TIME_STEP, cap, 120, 0.5, rng_seed=21,
                        slot0=slot0, external_reduce=True)
        set_all(h, ktq)
        h.set_state(p, ref_energy=ref_energy)
        h.set_record_rows(True)
        h.est_begin_block(nts)
        shards.append(h)
    a, b = shards
    part = [torch.zeros(2, dtype=torch.float64, device='cuda')
            for _ in range(3)]
    union, g1_confs = [], {}
    prev = (90, 30)
    for t in range(nts):
        perm = np.arange(prev[0] + prev[1])
        shift_b = prev[0]
        if t == 5:
            na, nb = a.num_walkers(), b.num_walkers()
            assert (na, nb) == prev and na > k
            buf = export(a, na - k, k)[0]
            a.set_num_walkers(na - k)
            b.import_walkers_at(nb, k, buf.data_ptr())
            # new union slot -> union slot before the transfer
            perm = np.concatenate([np.arange(na - k), na + np.arange(nb),
                                   np.arange(na - k, na)])
            shift_b = na - k
        a.step_local(part[0].data_ptr())
        b.step_local(part[1].data_ptr())
        torch.add(part[0], part[1], out=part[2])
        for h in shards:
            h.step_finish(part[2].data_ptr())
        for h in shards:
            h.step_estimators(t)
        (ca, ra, na), (cb, rb, nb) = walks.state_of(a), walks.state_of(b)
        ref = perm[np.concatenate([ra[:na], rb[:nb] + shift_b])]
        union.append((np.concatenate([ca[:na], cb[:nb]]), ref, na + nb))
        prev = (na, nb)
    dev = torch.device('cuda')
    slot_of = {e.key: e.slot for e in dmc_est.ESTIMATORS}
    got = {}
    for key in KEYS:
        parts = []
        for h in shards:
            ptr, width = h.est_rows_dev(slot_of[key])
            assert ptr and width
            parts.append(_wrap_f64(ptr, nts * width, dev).cpu().numpy()
                         .reshape(nts, width))
        got[key] = parts[0] + parts[1]
        if key in ('pair_dist', 'site'):
            # a / 3 + b / 3 is not (a + b) / 3 in floating point: add the
            # integers behind the quotients, which every entry gives back
            div = np.minimum(np.arange(nts) + 1.0, PFW)[:, None]
            counts = [np.rint(x * div) for x in parts]
            assert all(np.array_equal(c / div, x)
                       for c, x in zip(counts, parts))
            got[key] = (counts[0] + counts[1]) / div
    got['isf'] = got['isf'].reshape(nts, ktq[0], ktq[1] + 2)
    want = restate(union, shape)
    check_rows(got, want, 'union')
    assert all(np.abs(got[key][-2:]).max() > 0 for key in KEYS)
    # both shards took part, and the transfer mattered
    assert min(prev) > 20
    # g1: the definition on the union's configurations of the evaluated steps
    p, sh = model_dict(walks.spec(WALKS[shape]).cfc_spec), np.array(SHIFTS)
    for t in range(nts):
        if t % G1_STRIDE:
            assert not got['obdm'][t].any()
            continue
        confs = union[t][0]
        uniq, inv = np.unique(confs, axis=0, return_inverse=True)
        g = obdm.one_body_density(uniq, sh, p)[inv.reshape(-1)]
        bound = RTOL_G1 * np.maximum(1.0, np.abs(g)).sum(axis=0)
        err = np.abs(got['obdm'][t] - g.sum(axis=0))
        assert (err <= bound).all(), (t, err, bound)
        assert got['obdm'][t, 0] == union[t][2]         # a zero shift
    for h in (a, b, eng):
        h.close()


# ---- 5. a world of one equals the single-GPU block -------------------------

def _process_group():
    """A one-rank RCCL group as test_gpu_dist.py gets one, or None."""
    import socket
    import torch
    import torch.distributed as dist
    if not dist.is_available():
        return None
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    try:
        dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{port}',
                                rank=0, world_size=1,
                                device_id=torch.device('cuda', 0))
    except Exception as exc:            # no RCCL here: the plain path runs
        print('no process group:', exc)
        return None
    return dist


def test_world_of_one_reads_the_single_gpu_rows():
    import torch
    from phd_qmclib_amd.dist import DistributedDmc
    from phd_qmclib_amd.qmc_base import dmc_est
    shape = 'small'
    n, ktq = WALKS[shape].n, SHAPES[shape].ktq
    nts = 20
    spec = types.SimpleNamespace(as_pure_est=True, eval_stride=G1_STRIDE)
    table = {e.key: e for e in dmc_est.ESTIMATORS}
    group = _process_group()
    try:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            eng = walks.engine(WALKS[shape], stream=side.cuda_stream)
            a = make_ensemble(eng, shape)
            b = make_ensemble(eng, shape, external_reduce=True)
            for h in (a, b):
                set_all(h, ktq)
            dd = DistributedDmc(b, n, 'cuda', block_estimators=True,
                                force_collectives=group is not None)
            assert dd._collect == (group is not None)
            for blk in range(2):        # per-block resets included
                sa, ssf_a, dens_a = a.run_block_est(nts)
                sb, ssf_b, dens_b = dd.run_block(nts, estimators=True)
                assert np.array_equal(sa.energy, sb.energy)
                assert np.array_equal(sa.num_walkers, sb.num_walkers)
                assert np.array_equal(ssf_a, ssf_b)
                assert np.array_equal(dens_a[..., 0], dens_b)
                props = dd.global_props(sb)
                assert props.num_walkers.dtype == sb.num_walkers.dtype
                assert np.array_equal(props.num_walkers, sa.num_walkers)
                assert props.energy is sb.energy
                for key in KEYS:
                    est = table[key]
                    want = est.read(a, nts)
                    got = dd.read_estimator(key, nts)
                    assert got.shape == want.shape, key
                    assert got.tobytes() == want.tobytes(), key
                    assert np.abs(got[-2:]).max() > 0, key
                    # a second read does not sum the rows again
                    assert dd.read_estimator(key, nts).tobytes() == \
                        want.tobytes()
                    ta = est.reduce(want, sa, nts, False, spec)
                    tb = est.reduce(got, props, nts, False, spec)
                    assert len(ta) == len(tb) > 0
                    for x, y in zip(ta, tb):
                        assert np.array_equal(x, y), key
            a.close()
            b.close()
            eng.close()
    finally:
        if group is not None:
            group.destroy_process_group()


# ---- 6. opt-in -------------------------------------------------------------

SETTERS = {
    'pair distribution': lambda d: d.set_pair_dist_estimator(10, True, 3),
    'centre-of-mass diffusion': lambda d: d.set_cm_diffusion_estimator(True),
    r'F\(k, tau\)': lambda d: d.set_isf_estimator(3, 2, 2),
    'one-body density': lambda d: d.set_obdm_estimator(SHIFTS, 2),
    'site occupation': lambda d: d.set_site_estimator(4, 9, True, 3),
}


@pytest.mark.parametrize('phrase', list(SETTERS))
def test_block_estimators_are_opt_in(phrase):
    from phd_qmclib_amd.dist import DistributedDmc
    eng = make_engine('small')
    d = make_ensemble(eng, 'small', external_reduce=True)
    SETTERS[phrase](d)
    with pytest.raises(NotImplementedError, match=phrase) as exc:
        DistributedDmc(d, 16, 'cuda')
    assert 'block_estimators=True' in str(exc.value)
    assert not d.record_rows
    dd = DistributedDmc(d, 16, 'cuda', block_estimators=True)
    assert d.record_rows and dd.record_size() == d.walker_record_size()
    d.close()
    eng.close()
