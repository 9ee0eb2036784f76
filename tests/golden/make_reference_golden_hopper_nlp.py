"""Executes the REFERENCE'S OWN ``hopper/hopper.py`` NLP callbacks (g, gL_gU, jacrev(g), hess_lagrange_dot_g, model.f) and
records their inputs/outputs.

Build container only (needs the reference checkout; never runs on the GPU box, never imported by the product):

    python tests/golden/make_reference_golden_hopper_nlp.py     # rewrites tests/golden/ref_hopper_nlp.npz

Same method as ``make_reference_golden_drone_gaussian.py``: the script's text is read with ``ast`` AT RUN TIME -- the
module-level constants before ``class Model``, the class, and the closures ``g``, ``gL_gU``, ``lagrange_dot_g`` and
``hess_lagrange_dot_g`` of the solve block (:491-580) -- and executed unmodified on ``jax_standin``; nothing of it is stored
here.  ``f`` is taken through ``model.f`` (:441-453): the name ``f`` alone is ambiguous in the script (the solve block's
closure and its file handles).  The closures read the module globals ``model``, ``num_vars`` and ``nvar``, which are bound in
THIS script's namespace.  One library stand-in is bound here only (``jax_standin.py`` is untouched): ``jnp.array`` of a
NESTED list that holds traced scalars (the 2 x 4 matrices of :175-178 and :211-214; the stand-in's own stacks one level).
The friction fields are the script's own module-level draw after ``np.random.seed(1)`` (:33, :70-74) at the overridden M.

Two cases: S = 30, M = 30 with the script's phases 10 / 20 (keys without prefix) and S = 6, M = 4 with phases 2 / 4 (keys
``s6_*``), both at alpha = 0.2 and dt = T / S as the script computes it.  For each, at Z = make_reference_golden.hopper_Z and
a seeded mixed-sign lam: Z, lam, g for 'saa' and for 'baseline', jacrev(g) and hess_lagrange_dot_g(Z, lam) of the 'saa' model
as CSC triplets (the dense forms are not stored), gL, gU, f, the fields, the sizes and the SHA-256 of hopper/hopper.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jax_standin  # noqa: E402
import make_reference_golden as G  # noqa: E402

ALPHA = 0.2
OUT = os.path.join(HERE, "ref_hopper_nlp.npz")
NOTES = "reference text executed on jax_standin (torch fp64); closures g, gL_gU, lagrange_dot_g, hess_lagrange_dot_g; f = model.f"
CASES = (("", 30, 30, 10, 20), ("s6_", 6, 4, 2, 4))


def lam_mixed(ncon, seed=11):
    """mixed-sign multipliers of order one, one per row of g"""
    return np.random.RandomState(seed).uniform(-1.0, 1.0, ncon)


def _nested_array(jnp):
    """a copy of the stand-in's jnp whose ``array`` stacks nested lists of tensors and numbers"""
    import types
    import torch

    def stack(x):
        if isinstance(x, (list, tuple)):
            return torch.stack([stack(e) for e in x])
        return jax_standin._t(x)
    mine = types.ModuleType("jax.numpy")
    mine.__dict__.update({k: v for k, v in jnp.__dict__.items() if not k.startswith("__")})
    mine.array = lambda x, dtype=None: stack(x) if isinstance(x, (list, tuple)) else jnp.array(x)
    return mine


def record(jax, prefix, S, M, tj, tl, out):
    jnp = _nested_array(jax.numpy)
    ns = G.base_namespace(jax)
    ns["jnp"] = jnp
    np.random.seed(1)                                      # hopper.py:33; the fields are drawn at module level (:70-74)
    define = G.load_reference(os.path.join(G.REF, "hopper", "hopper.py"), ns,
                              overrides={"S": S, "M": M, "time_jump": tj, "time_land": tl},
                              nested=("g", "gL_gU", "lagrange_dot_g", "hess_lagrange_dot_g"))
    nvar = ns["num_vars"]
    assert ns["S"] == S and ns["M"] == M and nvar == 8 * (S + 1) + 4 * S + M + 2 and ns["dt"] == ns["T"] / S
    Model = ns["Model"]
    saa, base = Model(M, 'saa', ALPHA), Model(M, 'baseline', ALPHA)
    ns.update(model=saa, nvar=nvar)
    define()
    g, gL_gU, hess = ns["g"], ns["gL_gU"], ns["hess_lagrange_dot_g"]
    Z = G.hopper_Z(S, M, nvar)
    Zt = jnp.array(Z)
    gs = G.npy(g(Zt))
    lam = lam_mixed(gs.shape[0])
    g_L, g_U = gL_gU(Zt)
    J = G.npy(jax.jacrev(g)(Zt))
    H = G.npy(hess(Zt, jnp.array(lam)))
    f = float(saa.f(Zt))
    ns["model"] = base
    gs_base = G.npy(g(Zt))
    ns["model"] = saa
    out.update({prefix + "S": S, prefix + "M": M, prefix + "time_jump": tj, prefix + "time_land": tl, prefix + "dt": ns["dt"],
                prefix + "Z": Z, prefix + "lam": lam, prefix + "g_saa": gs, prefix + "g_baseline": gs_base,
                prefix + "gL": np.asarray(g_L), prefix + "gU": np.asarray(g_U), prefix + "f": f,
                prefix + "intensities": ns["intensities"], prefix + "thetas": ns["thetas"], prefix + "taus": ns["taus"]})
    out.update(G.csc_triplet(J, prefix + "J"))
    out.update(G.csc_triplet(H, prefix + "H"))
    print(prefix or "s30_", "nvar", nvar, "ncon", gs.shape[0], "nnz J", np.count_nonzero(J), "nnz H", np.count_nonzero(H))


def main():
    if not os.path.isdir(G.REF):
        raise SystemExit(f"{G.REF} not found: this generator only runs in the build container")
    jax = jax_standin.install()
    out = dict(alpha=ALPHA, notes=np.array(NOTES))
    for case in CASES:
        record(jax, *case, out)
    np.savez_compressed(OUT, **G.with_hashes(out, "hopper/hopper.py"))
    print(os.path.basename(OUT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
