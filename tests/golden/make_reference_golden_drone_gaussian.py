"""Executes the REFERENCE'S OWN ``drone/drone_gaussian.py`` callbacks (g, jacfwd(g), hess_lagrange_dot_g, gL_gU) and records
their inputs/outputs.

Build container only (needs the reference checkout; never runs on the GPU box, never imported by the product):

    python tests/golden/make_reference_golden_drone_gaussian.py     # rewrites tests/golden/ref_drone_gaussian_S20.npz

Same method as ``make_reference_golden_car_gaussian.py``: the script's text is read with ``ast`` AT RUN TIME -- the
module-level constants before ``class Model``, the class, and the closures ``g``, ``gL_gU``, ``lagrange_dot_g`` and
``hess_lagrange_dot_g`` of the solve block (:414-460) -- and executed unmodified on ``jax_standin``; nothing of it is stored
here.  ``drone_params`` is imported for real.  Library stand-ins, bound in THIS script's namespace only (``jax_standin.py``
is untouched):
  * ``fori_loop``: the stand-in's plain loop;
  * ``p_th_quantile_cdf_normal`` (drone_utils is ``scipy.stats.norm.ppf``, which ``torch.func`` cannot differentiate):
    ``torch.special.ndtri``, the same function with derivatives;
  * ``jnp.linalg.norm(x, 2)`` (:258 passes ``ord`` positionally, which the stand-in reads as an axis): ``torch.linalg.norm``
    with ``ord``.
The initial-guess file read (:104-116) is bypassed: Z is passed directly.  Recorded at alpha = 0.1 for S = 20 (keys
``<kind>_*``) and S = 5 (keys ``s5_<kind>_*``), kind in (wave, swerve) = tests/_drone_gaussian.us_wave / us_swerve with the
allocation alphas_spread: Z, the mean and covariance trajectories, g, jacfwd(g), hess_lagrange_dot_g(Z, lam_mixed), and gL_gU.
"""
import hashlib
import importlib
import os
import sys
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import jax_standin  # noqa: E402
import make_reference_golden as G  # noqa: E402
import _drone_gaussian as R  # noqa: E402  (the documented input builders only)

ALPHA = 0.1
OUT = os.path.join(HERE, "ref_drone_gaussian_S20.npz")
NOTES = ("reference text executed on jax_standin (torch fp64); library stand-ins: fori_loop = plain loop, "
         "p_th_quantile_cdf_normal = torch.special.ndtri (for scipy.stats.norm.ppf), jnp.linalg.norm with ord")


def record(jax, drone_params, S, prefix, out):
    import torch
    jnp = jax.numpy
    ns = G.base_namespace(jax)
    ns.update(drone_params=drone_params, fori_loop=jax.lax.fori_loop,
              p_th_quantile_cdf_normal=lambda p: torch.special.ndtri(jax_standin._t(p)))
    define = G.load_reference(os.path.join(G.REF, "drone", "drone_gaussian.py"), ns, overrides={"S": S},
                              nested=("g", "gL_gU", "lagrange_dot_g", "hess_lagrange_dot_g"))
    assert ns["S"] == S and ns["num_vars"] == R.sizes(S)[0]
    model = ns["Model"](S=S, alpha=ALPHA)
    ns.update(model=model, nvar=ns["num_vars"])
    define()
    g, gL_gU, hess = ns["g"], ns["gL_gU"], ns["hess_lagrange_dot_g"]
    n_nl = R.sizes(S)[1]
    for kind, us in (("wave", R.us_wave(S)), ("swerve", R.us_swerve(S))):
        Z = R.make_z(us, R.alphas_spread(S, ALPHA))
        Zt = jnp.array(Z)
        us_mat = model.convert_us_vec_to_us_mat(model.convert_z_to_variables(Zt)[0])
        gs = G.npy(g(Zt))
        lam = R.lam_mixed(gs.shape[0])
        g_L, g_U = gL_gU(Zt)
        out.update({f"{prefix}{kind}_Z": Z, f"{prefix}{kind}_us_mat": G.npy(us_mat),
                    f"{prefix}{kind}_xs": G.npy(model.us_to_state_trajectory(us_mat)),
                    f"{prefix}{kind}_Sigmas": G.npy(model.us_to_covariance_trajectory(us_mat)),
                    f"{prefix}{kind}_g": gs, f"{prefix}{kind}_jac": G.npy(jax.jacfwd(g)(Zt)), f"{prefix}{kind}_lam": lam,
                    f"{prefix}{kind}_hess": G.npy(hess(Zt, jnp.array(lam))),
                    f"{prefix}{kind}_gL": np.asarray(g_L), f"{prefix}{kind}_gU": np.asarray(g_U),
                    f"{prefix}{kind}_f": float(model.f(Zt))})
        assert gs.shape[0] == n_nl + ns["num_vars"] + 1


def main():
    if not os.path.isdir(G.REF):
        raise SystemExit(f"{G.REF} not found: this generator only runs in the build container")
    jax = jax_standin.install()
    import torch
    jax.numpy.linalg.norm = lambda x, ord=None, axis=None: torch.linalg.norm(jax_standin._t(x), ord=ord, dim=axis)
    sys.path.insert(0, os.path.join(G.REF, "drone"))
    drone_params = importlib.import_module("drone_params")
    out = dict(alpha=ALPHA, notes=np.array(NOTES))
    record(jax, drone_params, 20, "", out)
    record(jax, drone_params, 5, "s5_", out)
    for rel in ("drone/drone_gaussian.py", "drone/drone_utils.py"):
        digest = G.REF_SHA256.get(rel) or hashlib.sha256(Path(os.path.join(G.REF, rel)).read_bytes()).digest()
        out["gauss_sha256__" + rel.replace("/", "__").replace(".", "_")] = np.frombuffer(digest, dtype=np.uint8).copy()
    np.savez_compressed(OUT, **G.with_hashes(out, "drone/drone_params.py"))
    print(os.path.basename(OUT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
