"""Executes the REFERENCE'S OWN ``drone/drone_main_plot.py`` Monte-Carlo block and records its inputs/outputs.

Build container only (needs the reference checkout; never runs on the GPU box, never imported by the product):

    python tests/golden/make_reference_golden_main_plot.py     # rewrites tests/golden/ref_drone_main_plot_S20_M16.npz

Same method as ``make_reference_golden.py`` (whose helpers it imports): the script's text is read with ``ast`` AT RUN TIME --
the module-level constants before ``class Model``, the class, and the closures nested under ``if B_validate_monte_carlo:``
-- and executed unmodified on ``jax_standin``; nothing of it is stored here.  What runs:
  * ``Model.__init__``'s inline sampler (drone_main_plot.py:92-121) under ``np.random.seed(0)`` (:26), TWICE from the one
    stream as the script does (:603 the SAA batch, :632 the validation batch, no reseed in between);
  * ``Model.us_to_state_trajectories``, ``Model.obstacle_avoidance_constraints_euclidean`` (:254-269);
  * the closures ``monte_carlo_no_collisions_constraint_verification`` (:633-639) and ``monte_carlo_var`` (:640-652).
Sizes: the script's own S = 20; M_SAA = 8 draws first, then the M = 16 validation draws the fixture's outputs are for.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jax_standin  # noqa: E402
import make_reference_golden as G  # noqa: E402

S, M_SAA, M = 20, 8, 16
ALPHA = 0.1
OUT = os.path.join(HERE, f"ref_drone_main_plot_S{S}_M{M}.npz")


def controls(S):
    """a control sequence that steers past the obstacles at varying clearance (every row of every sample keeps
    (p-o)'Q(p-o) well above 1e-2: checked below, the GPU tests' tolerance degenerates at an obstacle's centre)"""
    t = np.arange(S)[:, None]
    return np.hstack([0.6 * np.cos(0.3 * t) + 0.3, 0.15 * np.sin(0.5 * t) + 0.02, 0.05 * np.cos(t)])


def main():
    if not os.path.isdir(G.REF):
        raise SystemExit(f"{G.REF} not found: this generator only runs in the build container")
    jax = jax_standin.install()
    jnp, vmap = jax.numpy, jax.vmap
    ns = G.base_namespace(jax)
    rel = os.path.join("drone", "drone_main_plot.py")
    closures = G.load_reference(os.path.join(G.REF, rel), ns, overrides={"S": S},
                                nested=("monte_carlo_no_collisions_constraint_verification", "monte_carlo_var"))
    assert ns["S"] == S and abs(ns["dt"] - ns["T"] / S) < 1e-15
    Model = ns["Model"]
    np.random.seed(0)                                              # drone_main_plot.py:26
    saa = Model(M_SAA, 'saa', ALPHA)                               # :603
    ns["M"] = M                                                    # :631 rebinds the module's M (the batched methods read it)
    model = Model(M)                                               # :632 -- the stream continues
    ns["model"] = model
    closures()
    us = jnp.array(controls(S))
    xs = model.us_to_state_trajectories(us)
    g = vmap(model.obstacle_avoidance_constraints_euclidean)(xs, model.obs_Qs)
    Us = jnp.repeat(us[None], M, axis=0)
    xs_mc, ok, Z = vmap(ns["monte_carlo_no_collisions_constraint_verification"])(Us, model.masses, model.DWs, model.obs_Qs)
    Z = G.npy(Z)
    a = (1.0 - G.npy(g)) ** 2
    assert a.min() > 1e-2, a.min()
    out = dict(S=S, M=M, M_saa=M_SAA, alpha=ALPHA, osqp_tol=float(ns["OSQP_TOL"]),
               saa_DWs=G.npy(saa.DWs), saa_masses=G.npy(saa.masses), saa_obs_Qs=G.npy(saa.obs_Qs),
               DWs=G.npy(model.DWs), masses=G.npy(model.masses), obs_Qs=G.npy(model.obs_Qs),
               us=G.npy(us), init_us=G.npy(model.initial_guess_us_mat()), xs=G.npy(xs), g=G.npy(g), xs_mc=G.npy(xs_mc),
               satisfied=G.npy(ok).astype(bool), Z=Z,
               var=float(ns["monte_carlo_var"](Z, ALPHA)), var_03=float(ns["monte_carlo_var"](Z, 0.3)))
    np.savez_compressed(OUT, **G.with_hashes(out, "drone/drone_main_plot.py"))
    print(os.path.basename(OUT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
