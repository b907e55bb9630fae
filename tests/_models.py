"""The models and the upload helper that the GPU tests share."""
from math import pi

import numpy as np


def box(n=16, cut=0.25, *, sites=None, ratio=1, depth=5 * pi ** 2, gint=2,
        **overrides):
    """The suite's lattice model: N bosons in `sites` lattice periods (default:
    one per boson), the contact cutoff at `cut` of the supercell.  `overrides`
    are `Spec` fields by their own names, applied last."""
    from phd_qmclib_amd.mrbp_qmc import Spec
    size = n if sites is None else sites
    args = dict(lattice_depth=depth, lattice_ratio=ratio,
                interaction_strength=gint, boson_number=n,
                supercell_size=size, tbf_contact_cutoff=cut * size)
    args.update(overrides)
    return Spec(**args)


def spec_from_golden(golden_params, tag):
    """The model of tests/golden/params.json[tag]."""
    from phd_qmclib_amd.mrbp_qmc import Spec
    return Spec(**golden_params[tag]['spec'])


def model_dict(cfc):
    """What tests/_obdm_restatement.py takes, from a CFCSpec."""
    return {'params': cfc.model_params._asdict(),
            'obf_params': cfc.obf_params._asdict(),
            'tbf_params': cfc.tbf_params._asdict()}


def _dev(eng, a):
    """Upload `a` as doubles to a `DeviceBuffer` on the engine's device."""
    from phd_qmclib_amd.engine import DeviceBuffer
    a = np.ascontiguousarray(a, dtype=np.float64)
    return DeviceBuffer(a.shape, eng.device).upload(a)
