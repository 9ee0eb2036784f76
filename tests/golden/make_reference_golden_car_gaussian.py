"""Executes the REFERENCE'S OWN ``car/driving_gaussian.py`` define step and records its inputs/outputs.

Build container only (needs the reference checkout; never runs on the GPU box, never imported by the product):

    python tests/golden/make_reference_golden_car_gaussian.py     # rewrites tests/golden/ref_driving_gaussian_S20.npz

Same method as ``make_reference_golden.py`` (whose helpers it imports): the script's text is read with ``ast`` AT RUN TIME --
the module-level constants before ``class Model`` and the class -- and executed unmodified on ``jax_standin``; nothing of it
is stored here.  ``driving_params`` is imported for real.  Library stand-ins, bound in THIS script's namespace only
(``jax_standin.py`` is untouched):
  * ``fori_loop``: the stand-in's plain loop;
  * ``p_th_quantile_cdf_normal`` (driving_utils.py:6-7 is ``scipy.stats.norm.ppf``, which ``torch.func`` cannot
    differentiate): ``torch.special.ndtri``, the same function with a derivative -- a library stand-in like the others;
  * ``jnp.block`` (used once, for the block-diagonal initial covariance, :88-91): ``torch.cat`` of the rows.
What runs, for both control sequences (``guess`` = the reference's initial guess, ``steer``) with the uniform allocation
alpha / S at alpha = 0.05: us_to_state_trajectory, us_to_covariance_trajectory, separation_distances_at_all_times, the five
outputs of get_all_constraints_coeffs, get_control_risk_constraints_coeffs_all, get_constraints_coeffs at scp_iter 0 and 2.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jax_standin  # noqa: E402
import make_reference_golden as G  # noqa: E402

S, ALPHA = 20, 0.05
OUT = os.path.join(HERE, f"ref_driving_gaussian_S{S}.npz")
NOTES = ("reference text executed on jax_standin (torch fp64); library stand-ins: fori_loop = plain loop, "
         "p_th_quantile_cdf_normal = torch.special.ndtri (for scipy.stats.norm.ppf), jnp.block = torch.cat")


def steer(S):
    t = np.arange(S, dtype=np.float64)
    return np.stack([0.3 * np.cos(0.4 * t), 0.05 * np.sin(0.3 * t) + 0.02], axis=1)


def main():
    import torch
    if not os.path.isdir(G.REF):
        raise SystemExit(f"{G.REF} not found: this generator only runs in the build container")
    jax = jax_standin.install()
    jnp = jax.numpy
    jnp.block = lambda rows: torch.cat([torch.cat([jax_standin._t(b) for b in row], dim=1) for row in rows], dim=0)
    sys.path.insert(0, os.path.join(G.REF, "car"))
    driving_params = importlib.import_module("driving_params")
    ns = G.base_namespace(jax)
    ns.update(driving_params=driving_params, fori_loop=jax.lax.fori_loop,
              p_th_quantile_cdf_normal=lambda p: torch.special.ndtri(jax_standin._t(p)))
    dt = driving_params.T / S
    G.load_reference(os.path.join(G.REF, "car", "driving_gaussian.py"), ns, overrides={"S": S, "dt": dt})
    assert ns["S"] == S and ns["dt"] == dt and ns["OSQP_TOL"] == 1e-8
    model = ns["Model"](alpha=ALPHA)
    alphas = model.initial_guess_alphas_risk()
    out = dict(S=S, alpha=ALPHA, dt=dt, osqp_tol=float(ns["OSQP_TOL"]), alphas_risk=G.npy(alphas), notes=np.array(NOTES))
    A, l, u = model.get_control_risk_constraints_coeffs_all()
    out.update(con_A=G.npy(A), con_l=G.npy(l), con_u=G.npy(u))
    for kind in ("guess", "steer"):
        us = model.initial_guess_us_mat() if kind == "guess" else jnp.array(steer(S))
        xs = model.us_to_state_trajectory(us)
        Sigmas = model.us_to_covariance_trajectory(us)
        dist = model.separation_distances_at_all_times(xs, Sigmas, alphas)
        fdu, flo, fup, gdu, gup = model.get_all_constraints_coeffs(us, alphas)
        out.update({f"{kind}_us": G.npy(us), f"{kind}_xs": G.npy(xs), f"{kind}_Sigmas": G.npy(Sigmas),
                    f"{kind}_dist": G.npy(dist), f"{kind}_final_du_dalphas": G.npy(fdu), f"{kind}_final_low": G.npy(flo),
                    f"{kind}_final_up": G.npy(fup), f"{kind}_g_obs_du_dalphas": G.npy(gdu), f"{kind}_g_up": G.npy(gup)})
        for it in (0, 2):
            with np.errstate(invalid="ignore"):                 # `ls[n_x:] *= 0` turns -inf into nan (:416-420)
                A, l, u = model.get_constraints_coeffs(us, alphas, it)
            out.update({f"{kind}_qp{it}_A": A.toarray(), f"{kind}_qp{it}_l": l, f"{kind}_qp{it}_u": u})
    # test_reference_pin.py re-hashes every `ref_sha256__*` key of every ref_*.npz against a fixed list of files that
    # driving_gaussian.py is not on: the digests of this fixture's own sources go under `gauss_sha256__*`
    # (test_car_gaussian_pin.py re-hashes those)
    import hashlib
    from pathlib import Path
    for rel in ("car/driving_gaussian.py", "car/driving_utils.py"):
        digest = G.REF_SHA256.get(rel) or hashlib.sha256(Path(os.path.join(G.REF, rel)).read_bytes()).digest()
        out["gauss_sha256__" + rel.replace("/", "__").replace(".", "_")] = np.frombuffer(digest, dtype=np.uint8).copy()
    np.savez_compressed(OUT, **G.with_hashes(out, "car/driving_params.py"))
    print(os.path.basename(OUT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
