"""Runs the README quick-start snippet (smaller sizes) -- development check."""
import os
import sys
from itertools import islice
from math import pi

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phd_qmclib_amd import mrbp_qmc  # noqa

spec = mrbp_qmc.Spec(lattice_depth=5 * pi**2, lattice_ratio=1, interaction_strength=2,
                     boson_number=64, supercell_size=64, tbf_contact_cutoff=16)
vmc = mrbp_qmc.vmc.EnsembleSampling(spec, move_spread=0.125, num_chains=1 << 12, rng_seed=1)
vmc.init_random(seed=0)
for blk in islice(vmc.blocks(64), 2):
    print(blk.energy.mean() / 64, blk.accept_rate.mean())
shifts, g1, g1_err = vmc.one_body_density(np.linspace(0, 32, 17))   # one-body density matrix g1(s)
r, g2, g2_err = vmc.pair_distribution(64)                            # pair distribution function g2(r)
dmc = mrbp_qmc.dmc.Sampling(spec, time_step=6.25e-4, max_num_walkers=4400,
                            target_num_walkers=4096, num_walkers_control_factor=0.5, rng_seed=1,
                            pair_dist_est_spec=mrbp_qmc.dmc.PairDistEstSpec(64, pfw_num_time_steps=32),
                            obdm_est_spec=mrbp_qmc.dmc.OBDMEstSpec(shifts, eval_stride=16))   # mixed g1(s), every 16th step
confs = np.zeros((4096, 2, 64)); confs[:, 0] = vmc.confs()
for blk in islice(dmc.blocks(dmc.build_state(confs), 32, 1), 2):
    print(blk.iter_props.energy.sum() / blk.iter_props.weight.sum() / 64)
    g2_pure = blk.iter_pair_dist[-1] / blk.iter_props.num_walkers[-1]   # pure g2(r) histogram at dmc.pair_dist_bins
    g1_dmc = blk.iter_obdm[::16].sum(axis=0) / blk.iter_props.num_walkers[::16].sum()   # mixed g1(s) (zero in the burn-in block)
print('g1(0) =', g1_dmc[0], ' extrapolated g1(s):', 2 * g1_dmc - g1)   # 2 DMC - VMC
assert g1_dmc[0] == 1.0
print('README snippet OK')
