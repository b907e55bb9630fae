"""One-body density matrix: the checks that need no GPU.

* the NumPy restatement of the definition (tests/_obdm_restatement.py), which
  the GPU tests use for batch shapes the pure-Python reference is too slow
  for, against the reference's golden values (tests/golden/obdm.npz, written
  by tools/gen_obdm_golden.py) with the suite's criterion
  |delta| <= 2e-11 max(1, |x|);
* the ctypes binding declares the four entry points with the argument types
  of include/qmcwalk.h;
* `mrbp_qmc.PhysicalFuncs` is importable without a GPU.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ._obdm_restatement import ith_one_body_density
from .conftest import GOLDEN, ROOT

RTOL = 2e-11
OBDM_ENTRIES = ('qmc_obdm', 'qmc_obdm_dev', 'qmc_obdm_reduce_dev',
                'qmc_vmc_obdm')


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))


@pytest.fixture(scope='module')
def golden_obdm():
    return np.load(os.path.join(GOLDEN, 'obdm.npz'), allow_pickle=False)


def test_golden_covers_every_spec(golden_params, golden_obdm, golden_kernels):
    tags = {k.split('/')[0] for k in golden_obdm.files}
    assert tags == set(golden_params) and len(tags) == 15
    for tag in tags:
        n = golden_params[tag]['params']['boson_number']
        g1, sh = golden_obdm[tag + '/g1'], golden_obdm[tag + '/shifts']
        assert np.all(np.isfinite(g1)) and g1.shape[1] == len(sh)
        assert (tag + '/ith' in golden_obdm.files) == (n <= 64)
        if n < 512:
            assert len(g1) == len(golden_kernels[tag + '/pos'])
            assert len(sh) == 15
        else:
            assert g1.shape == (2, 6)


def test_restatement_matches_reference_golden(golden_params, golden_kernels,
                                              golden_obdm):
    for tag in sorted(golden_params):
        g1 = golden_obdm[tag + '/g1']
        pos = golden_kernels[tag + '/pos'][:len(g1)]
        ith = ith_one_body_density(pos, golden_obdm[tag + '/shifts'],
                                   golden_params[tag])
        assert close(ith.mean(axis=2), g1), tag
        if tag + '/ith' in golden_obdm.files:
            ref = golden_obdm[tag + '/ith']
            assert np.all(np.isfinite(ref))
            assert close(ith, ref), tag


_CTYPES = {'qmc_engine*': C.c_void_p, 'qmc_vmc*': C.c_void_p,
           'int64_t': C.c_int64, 'int32_t': C.c_int32}


def test_binding_matches_header():
    from phd_qmclib_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'qmcwalk.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    for name in OBDM_ENTRIES:
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, text)
        assert m, name + ' is not declared in include/qmcwalk.h'
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int
        params = [' '.join(p.split()) for p in m.group(1).split(',')]
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            typ = re.sub(r'\s*\*\s*', '*', p.rsplit(' ', 1)[0] if '*' not in
                         p.rsplit(' ', 1)[-1] else
                         p[:p.rindex('*') + 1]).replace('const ', '')
            if typ == 'double*':
                # host arrays are typed pointers, device addresses void*
                assert a in (_lib._dp, C.c_void_p), (name, p)
                host = name in ('qmc_obdm', 'qmc_vmc_obdm')
                assert a is (_lib._dp if host else C.c_void_p), (name, p)
            else:
                assert a is _CTYPES[typ], (name, p)


def test_physical_funcs_importable_without_gpu(golden_params, monkeypatch,
                                               tmp_path):
    from phd_qmclib_amd import _lib, mrbp_qmc
    spec = mrbp_qmc.Spec(**golden_params['box16']['spec'])
    pf = mrbp_qmc.PhysicalFuncs.from_model_spec(spec)
    assert pf.cfc_spec_nt == spec.cfc_spec
    assert pf.core_funcs is mrbp_qmc.core_funcs
    for name in ('wf_abs_log', 'energy', 'one_body_density', 'fourier_density'):
        assert callable(getattr(pf, name))
    assert callable(mrbp_qmc.core_funcs.one_body_density)
    assert callable(mrbp_qmc.core_funcs.ith_one_body_density)
    # the host-side member works with no library at all ...
    conf = np.zeros((2, 16))
    conf[0] = np.arange(16) + 0.25
    kz = np.array([0.0, 0.5, 2.0])
    fd = pf.fourier_density(kz, conf)
    assert fd.shape == (3,) and fd.dtype == np.complex128
    assert np.allclose(fd, np.exp(1j * kz[:, None] * conf[0][None, :]).sum(1),
                       rtol=0, atol=1e-12)
    # ... and a device member raises the loader's usual error only when called
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'libqmcwalk.so'))
    monkeypatch.setattr(mrbp_qmc.core_funcs, '_engines', {})
    with pytest.raises(_lib.QmcError, match='has not been built'):
        pf.one_body_density(0.5, conf)
