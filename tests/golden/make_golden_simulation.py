"""
Generates tests/golden/simulation_case.npz by running the REFERENCE's own shape.py / sdf.py / util.py in the build container (needs
/root/reference and oracle/_ref, see oracle/ref_harness.py).  Data only: seeded points, the reference's signed distances and
sdf_normals there, and quantiles of the reference's loc_error.  Re-run with

    python tests/golden/make_golden_simulation.py

The reference's IntersectionShape cannot be constructed (its __init__ calls Shape.__init__ without self, shape.py:424): the instance is
made with object.__new__ and given the attributes its constructor would set; its `sdf` method -- the arithmetic that is pinned -- runs
unmodified.
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_harness                                    # noqa: E402

N_SIGMA = 200000
SIGMA_KW = dict(psf_width=(280, 280, 840), mean_photon_count=600, bg_photon_count=20)


def main():
    sh = ref_harness.load_shapes()
    from ch_shrinkwrap import sdf as ref_sdf, util as ref_util
    rng = np.random.default_rng(2025)
    P = rng.uniform(-1.0, 1.0, size=(2000, 3)) * np.array([520.0, 420.0, 130.0])[None, :]
    inter = object.__new__(sh.IntersectionShape)
    sh.Shape.__init__(inter)
    inter._s0, inter._s1, inter._k = sh.Sphere(radius=150.0), sh.Box(np.array([100.0, 120.0, 80.0]), 10.0), 15.0
    shapes = {
        'torus': sh.Torus(radius=100.0, r=30.0, centroid=np.array([10.0, -20.0, 5.0])),
        'two_toruses': sh.TwoToruses(r=30, R=100),
        'n_toruses': sh.NToruses({'one': {'r': 30.0, 'R': 100.0}, 'two': {'r': 10.0, 'R': 75.0}, 'three': {'r': 30.0, 'R': 150.0}}),
        'dual_capsule': sh.DualCapsule(length=400.0, r=40.0, sep=150.0),
        'intersection': inter,
    }
    out = dict(points=P)
    for name, s in shapes.items():
        out['sdf_' + name] = s.sdf(P.T)
        out['normals_' + name] = ref_sdf.sdf_normals(P.T, s.sdf).T
    np.random.seed(20251017)
    sigma = ref_util.loc_error((N_SIGMA, 3), 'exponential', **SIGMA_KW)
    assert sigma.shape == (N_SIGMA, 3)
    out['sigma_quantiles'] = np.stack([np.quantile(sigma[:, a], np.arange(1, 1000) / 1000.0) for a in range(3)], 1)      # (999, 3)
    out['sigma_n'] = np.int64(N_SIGMA)
    np.savez_compressed(os.path.join(HERE, 'simulation_case.npz'), **out)
    print('wrote simulation_case.npz:', {k: np.shape(v) for k, v in out.items()})


if __name__ == '__main__':
    main()
