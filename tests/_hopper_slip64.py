"""Shared by the fp64 slip-row tests (CPU and GPU): the fp64 reference of every output of csrc/hopper_slip64.hip, from
oracle/hopper.py, for K problems and any phase times."""
import numpy as np

import _hopper_nlp as R

ALPHA = 0.2
MU_NOM = 0.10


def phase_cases(S):
    """default, no first phase, no second phase, no contacts, (and for the GPU sweep) every step in contact"""
    tj, tl = S // 3, (2 * S) // 3
    return {"default": (tj, tl), "no first phase": (0, tl), "no second phase": (tj, S), "no contacts": (0, S), "all contact": (S, S)}


def oracle(fields, S, phases, method="saa"):
    from oracle import hopper as oh
    o = oh.Model(*fields, method=method, alpha=ALPHA, S=S)
    o.time_jump, o.time_land = phases
    return o


def layout(S, M, phases, method="saa"):
    return R.layout(S, M, phases[0], phases[1], method)


def inputs(S, M, K, phases, seed=0):
    """fields (M, 30) x 3, Zs (K, nvar), lams (K, ncon) of mixed sign, add (K, S+1, 78)"""
    from oracle import hopper as oh
    rng = np.random.RandomState(100 + 7 * S + M + seed)
    fields = oh.sample_friction_fields(rng, M)
    Zs = np.stack([R.problem(S, M, seed + k) for k in range(K)])
    ncon = layout(S, M, phases)["ncon"]
    lams = rng.uniform(-1, 1, (K, ncon))
    add = rng.uniform(-3, 3, (K, S + 1, 78))
    return fields, Zs, lams, add


def reference(fields, Zs, lams, add, S, phases, method="saa"):
    """-> dict of fp64 arrays in the kernels' layouts: h, dh_dfz (K, C, M), dh_dx (K, C, 3, M), Zmax (K, M), D1, D2, D0 (K, C),
    terms (K, C, 3): sum_i |lam term| of the three sums, add (K, S+1, 78) = add + the slip share of hess(lam . g)"""
    o = oracle(fields, S, phases, method)
    M, K = o.M, Zs.shape[0]
    L = layout(S, M, phases, method)
    C = L["C"]
    r0 = L["risk"] + (1 + M if method == "saa" else 0)
    out = {k: [] for k in ("h", "dh_dfz", "dh_dx", "Zmax", "D1", "D2", "D0", "terms", "add")}
    for k in range(K):
        Z = Zs[k]
        px, forces = o.contact_inputs(Z)
        h, dfz, dpx = o.slip_partials(px, forces)                                   # (M, C)
        Jee, _ = o.contact_chain(Z)
        out["h"].append(h.T), out["dh_dfz"].append(dfz.T)
        out["dh_dx"].append(dpx.T[:, None, :] * Jee[:, :, None])
        out["Zmax"].append(h.max(axis=1) if C else np.full(M, -np.inf))
        lam_s = lams[k][r0:r0 + M * C].reshape(M, C)
        D1, D2 = o.slip_hessian_sums(px, forces, lam_s)
        D0 = np.sum(lam_s * dpx, axis=0)
        from oracle.hopper import friction_derivatives, hessian_from_sums
        _, dmu, d2mu = friction_derivatives(px, o.intensities, o.thetas, o.taus)
        out["terms"].append(np.stack([np.sum(np.abs(lam_s * dmu), 0), np.abs(forces[:, 1]) * np.sum(np.abs(lam_s * d2mu), 0),
                                      np.sum(np.abs(lam_s * dpx), 0)], -1))
        out["D1"].append(D1), out["D2"].append(D2), out["D0"].append(D0)
        Hs = hessian_from_sums(o, Z, D0, D1, D2).toarray() if C else np.zeros((o.num_vars, o.num_vars))
        blocks, rest = R.blocks_from_dense(Hs, S)
        assert not np.any(rest)
        out["add"].append(add[k] + R.tril78(blocks))
    return {k: np.stack(v) for k, v in out.items()}


def errors(got, ref):
    """relative to each array's max |entry|; the Hessian share ("add", computed into a zeroed add) per step block, where a
    block that is exactly 0 in the reference must be exactly 0"""
    errs = {}
    for name in ("h", "dh_dfz", "dh_dx", "Zmax", "D1", "D2", "D0"):
        if got.get(name) is not None and ref["h"].size:           # without a contact step nothing is written
            assert got[name].shape == ref[name].shape and np.all(np.isfinite(got[name])), name
            errs[name] = R.rel_err(got[name], ref[name])
    if got.get("add") is not None:
        errs["hess"] = R.rel_err_blocks(got["add"], ref["add"], 1)
    return errs


def split_D(D):
    """(K, C, 3) -> dict D1, D2, D0"""
    return {"D1": D[..., 0], "D2": D[..., 1], "D0": D[..., 2]}
