"""The surface of the drone and driving ``Model`` facades that bench.py, scp_bench.py, tools/ and the tests reach into:
both are subclasses of ``_saa_model.SaaModel``, every name keeps the call shapes its callers use, and the state the base
creates covers what it later drops.  No device, no Model instance."""
import inspect
import types

import pytest

from riskaversetrajopt_amd import _saa_model, cvar_cuts, driving, drone_risk

MODELS = {"drone": drone_risk.Model, "driving": driving.Model}

# name -> the positional call shapes (after self) that must bind
CALLS = {
    "drone": {
        "_us_device": [("us",)],
        "_inputs": [(None,)],
        "_params": [("M", "ld"), ("M", "ld", "rows_out")],
        "_params_key": [("M", "ld"), ("M", "ld", "rows_out")],
        "_params_build": [("M", "ld"), ("M", "ld", "rows_out")],
        "_tiled_noise": [("dW", "M", "ld")],
        "_native_define_buffers": [("cs",)],
        "_native_loop_solver": [(), ("min_S",)],
        "_reduced_cut_solver": [("M",), ("M", "ld")],
    },
    "driving": {
        "_us_device": [("us",)],
        "_params": [("M",)],
        "_params_key": [("M",), ("M", "rows_out")],
        "_params_build": [("M",), ("M", "rows_out")],
        "_tiled_noise": [("dW", "M"), ("dW", "M", "ld")],
        "_native_loop_solver": [()],
        "_reduced_cut_solver": [("M",), ("M", "ld")],
        "_goal64": [()],
    },
}
# attributes an instance gets from __init__ / from_device (the batch in kernel layout)
BATCH = {"drone": ("_mass", "_dW"), "driving": ("_dW", "_ws", "_x0", "_wr")}
LAZY = ("_world", "_group", "_cut_solver", "_gen_buffers", "_lin_buffers", "_define_host", "_fast", "_dW_tiled_cache",
        "_native_define", "_rollout_params", "_noise_seed", "_sampler_dt", "_params_cache")


def _state(method):
    ns = types.SimpleNamespace()
    method(ns)
    return vars(ns)


@pytest.mark.parametrize("system", sorted(MODELS))
def test_model_is_a_subclass_of_the_shared_base(system):
    assert issubclass(MODELS[system], _saa_model.SaaModel) and MODELS[system] is not _saa_model.SaaModel


@pytest.mark.parametrize("system,name", [(s, n) for s in sorted(CALLS) for n in sorted(CALLS[s])])
def test_private_method_keeps_its_call_shapes(system, name):
    fn = getattr(MODELS[system], name)
    assert callable(fn)
    for args in CALLS[system][name]:
        inspect.signature(fn).bind("self", *args)           # TypeError if the call shape no longer fits
    n_max = max(len(a) for a in CALLS[system][name])
    if name not in ("_params",):                            # (_params forwards *args to _params_key / _params_build)
        with pytest.raises(TypeError):
            inspect.signature(fn).bind("self", *range(n_max + 1))


@pytest.mark.parametrize("system", sorted(MODELS))
def test_instance_state_and_switches(system, monkeypatch):
    cls = MODELS[system]
    created = _state(cls._init_state)
    assert set(LAZY) <= set(created)
    assert created["_cut_solver"] is None and created["_native_define"] is None and created["_world"] == 1
    assert created["_params_cache"] == {}
    stored = set(cls.__init__.__code__.co_names) | set(cls.from_device.__func__.__code__.co_names)
    assert set(BATCH[system]) <= stored and "check_finite" in stored
    assert "check_finite" in inspect.signature(cls.__init__).parameters
    assert cls.TILED_NOISE is True
    other = MODELS["driving" if system == "drone" else "drone"]
    monkeypatch.setattr(cls, "TILED_NOISE", False)                          # settable on either subclass alone
    assert other.TILED_NOISE is True and _saa_model.SaaModel.TILED_NOISE is True
    for name in ("N_U", "N_NOISE", "PARAMS", "KAPPA", "CUT_ROWS", "CUT_RHS0", "RCOST", "SLACK_PENALTY"):
        assert getattr(cls, name) is not None, name


def test_init_state_names_everything_drop_solver_state_clears():
    dropped = _state(_saa_model.SaaModel._drop_solver_state)
    created = _state(_saa_model.SaaModel._init_state)
    assert dropped and set(dropped) <= set(created)
    assert all(v is None for v in dropped.values()) and all(created[k] is None for k in dropped)
    for cls in MODELS.values():                                             # one copy each: nothing re-implemented below
        for name in ("_init_state", "_drop_solver_state", "shard", "mc_step_device", "set_noise", "invalidate_noise",
                     "certify_reduced", "_us_device", "_empty", "_reuse", "convert_us_vec_to_us_mat",
                     "convert_us_mat_to_us_jaxvec", "monte_carlo_statistics", "monte_carlo_avar"):
            assert name not in vars(cls), (cls, name)


def test_public_signatures_are_the_facades_own():
    d, c = drone_risk.Model, driving.Model
    assert inspect.signature(d.solve).parameters["verbose"].default is True
    assert inspect.signature(c.solve).parameters["verbose"].default is False
    assert list(inspect.signature(d.from_device).parameters) == ["S", "dW", "mass", "Qsym", "method", "alpha", "M",
                                                                 "noise_seed", "sampler_dt"]
    assert list(inspect.signature(c.from_device).parameters) == ["S", "dW", "x0_ped", "w_speed", "w_rep", "method", "alpha",
                                                                 "noise_seed"]
    assert c.SCP_NATIVE_LOOP_DEFAULT is False and c.SCP_NATIVE_ENTRY == "rato_scp_run_car"
    assert callable(d.monte_carlo_no_collisions_constraint_verification)
    assert callable(c.monte_carlo_separation_constraints_verification)
    for mod in (drone_risk, driving):
        p = inspect.signature(mod.scp_run_native_batch).parameters
        assert list(p)[:3] == ["models", "us0", "iters"] and p["n_threads"].default == 16 and p["check_finite"].default is True
        inspect.signature(mod._check_batch).bind([])
    assert inspect.signature(drone_risk.scp_run_native_batch).parameters["first_cvar"].default == 2
    assert inspect.signature(driving.scp_run_native_batch).parameters["first_cvar"].default == 1


def test_cut_solver_keeps_what_the_facades_and_tests_call():
    for name in ("evaluate", "set_linearization_point", "begin", "enqueue_relinearize", "relinearize_kept_cuts", "solve",
                 "native_loop_applies", "_native_solver", "_native_destroy", "_keep_arrays", "_follow_native", "_solve_native",
                 "_solve"):
        assert callable(getattr(cvar_cuts.CvarCutSolver, name)), name
    for name in ("scp_run", "check_scp_batch", "scp_batch_inputs", "scp_batch_run", "scp_run_native_batch"):
        assert callable(getattr(cvar_cuts, name)), name
