"""CPU-only: the Python side of the float64 register family's form table (`solver.F64_FORMS`) against literals
written out here, not derived from it: which C entry point and flag bits a `force` name selects, and the surface of the
functions bound from the table -- names, parameter lists with defaults, docstrings that name their C entry points."""
import inspect

import pytest

from pybold_amd import _lib, solver, torch_ops

HOST_TEXT = ("float64 y: force must be None, 'fast' (register-resident float64 kernel, one problem per wave), 'generic' (LDS "
             "kernel), 'long_hrf' (the register form for HRFs of up to 48 taps, up to 640 scans) or 'split_long_hrf' (the same "
             "over four waves, 641..1280 scans)")
PP_TEXT = ("float64 y: force must be None, 'fast' (register-resident float64 kernel, one problem per wave), 'split' (the same "
           "over four waves, 641..1280 scans), 'generic' (LDS kernel), 'long_hrf' (one problem per wave, HRFs of up to 48 taps) "
           "or 'split_long_hrf' (four waves, 641..1280 scans, HRFs of up to 48 taps)")
SPLIT_TEXT = "force='split' names the four-wave form with one HRF per problem: fista_solve_pp_d only"

# force: (taps on the host -- fista_solve on a float64 Y --, one HRF per problem -- fista_solve_pp_d); a string: the ValueError
ROUTES = {
    None: (("pb_fista_solve_d", 0), ("pb_fista_solve_pp_d", 0)),
    "generic": (("pb_fista_solve_d", _lib.PB_FLAG_FORCE_GENERIC), ("pb_fista_solve_pp_d", _lib.PB_FLAG_FORCE_GENERIC)),
    "fast": (("pb_fista_solve_d", _lib.PB_FLAG_FORCE_FAST), ("pb_fista_solve_pp_d", _lib.PB_FLAG_FORCE_FAST)),
    "split": (SPLIT_TEXT, ("pb_fista_solve_pp_d", _lib.PB_FLAG_PP_SPLIT)),
    "long_hrf": (("pb_fista_solve_d", _lib.PB_FLAG_LONG_HRF), ("pb_fista_solve_pp_d", _lib.PB_FLAG_LONG_HRF)),
    "split_long_hrf": (("pb_fista_solve_split_long_d", 0), ("pb_fista_solve_split_long_pp_d", 0)),
    "mfma": (HOST_TEXT, PP_TEXT),                    # a float32 form's name
    "device_split": (HOST_TEXT, PP_TEXT),            # no form's name
}


@pytest.mark.parametrize("force", list(ROUTES), ids=str)
@pytest.mark.parametrize("pp", (False, True), ids=("host_taps", "pp"))
def test_the_solve_route_of_every_force_name(force, pp):
    want = ROUTES[force][pp]
    if isinstance(want, str):
        with pytest.raises(ValueError) as e:
            solver._f64_solve_route(force, pp)
        assert str(e.value) == want
    else:
        assert solver._f64_solve_route(force, pp) == want


def test_the_opt_in_names_stay_out_of_the_float32_table():
    assert not {"split", "long_hrf", "split_long_hrf"} & set(solver._FORCE)
    assert _lib.PB_FLAG_FORCE_GENERIC == 1 and _lib.PB_FLAG_FORCE_FAST == 2
    assert _lib.PB_FLAG_PP_SPLIT == 1 << 20 and _lib.PB_FLAG_LONG_HRF == 1 << 21


TAIL = [("sigma", inspect.Parameter.empty), ("early_stopping", True), ("tol", 1.0e-6), ("wind", 6), ("nb_iter", 1000),
        ("nb_sub_iter", 1000), ("outer_chunk", 0), ("W0", None), ("want_trace", True)]
HOST_PARAMS = [("Y", inspect.Parameter.empty), ("hrf", inspect.Parameter.empty), ("step", inspect.Parameter.empty)] + TAIL
PP_PARAMS = [("Y", inspect.Parameter.empty), ("taps", inspect.Parameter.empty), ("steps", inspect.Parameter.empty)] + TAIL
SEARCHES = {"auto_lbda_solve": "pb_auto_lbda_d", "auto_lbda_solve_split": "pb_auto_lbda_split_d",
            "auto_lbda_solve_long": "pb_auto_lbda_long_d", "auto_lbda_solve_split_long": "pb_auto_lbda_split_long_d",
            "auto_lbda_solve_pp": "pb_auto_lbda_pp_d", "auto_lbda_solve_split_pp": "pb_auto_lbda_split_pp_d",
            "auto_lbda_solve_long_pp": "pb_auto_lbda_long_pp_d", "auto_lbda_solve_split_long_pp": "pb_auto_lbda_split_long_pp_d"}
QUERIES = {"pp_split_supported": ("pb_fista_pp_split_supported", True), "long_hrf_supported": ("pb_fista_long_hrf_supported", True),
           "split_long_hrf_supported": ("pb_fista_split_long_hrf_supported", True),
           "auto_lbda_supported": ("pb_auto_lbda_supported", False), "auto_lbda_split_supported": ("pb_auto_lbda_split_supported", False),
           "auto_lbda_long_supported": ("pb_auto_lbda_long_supported", False),
           "auto_lbda_split_long_supported": ("pb_auto_lbda_split_long_supported", False)}


def params(fn):
    sig = inspect.signature(fn)
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    return [(p.name, p.default) for p in sig.parameters.values()]


def test_the_bound_searches_keep_their_parameter_lists():
    for name in SEARCHES:
        assert params(getattr(solver, name)) == (PP_PARAMS if name.endswith("_pp") else HOST_PARAMS), name
        assert getattr(solver, name).__name__ == name
    for name in ("auto_lbda_solve", "auto_lbda_solve_split", "auto_lbda_solve_long", "auto_lbda_solve_split_long"):
        assert params(getattr(torch_ops, name)) == HOST_PARAMS, name
        assert getattr(torch_ops, name).__name__ == name and ("torch.ops.pybold_hip.%s``" % name) in getattr(torch_ops, name).__doc__


def test_the_bound_functions_say_what_they_call():
    for name, entry in SEARCHES.items():
        doc = getattr(solver, name).__doc__
        assert doc and doc.strip() and ("``%s``" % entry in doc or "``%s:" % entry in doc or "``%s;" % entry in doc), name
    for name, (query, with_stop) in QUERIES.items():
        fn = getattr(solver, name)
        assert fn.__doc__ and ("``%s``" % query in fn.__doc__ or "``%s:" % query in fn.__doc__), name
        want = [("n_scans", inspect.Parameter.empty), ("n_taps", inspect.Parameter.empty)]
        assert params(fn) == want + ([("stop", None)] if with_stop else []) + [("wind", 6)] and fn.__name__ == name, name


def test_every_name_of_the_table_is_bound_and_known_to_the_library():
    assert list(solver.F64_FORMS) == ["one_wave", "four_waves", "long", "four_waves_long"]
    bound = [n for f in solver.F64_FORMS.values() for n in f.public if n]
    assert sorted(bound) == sorted(list(SEARCHES) + list(QUERIES))
    for f in solver.F64_FORMS.values():
        entries = [f.search, f.search_pp, f.search_query] + [r[0] for r in (f.solve, f.solve_pp) if r] + ([f.solve_query] if f.solve_query else [])
        assert all(e in _lib.SIGNATURES for e in entries), f.key
        assert SEARCHES[f.public.search] == f.search and SEARCHES[f.public.search_pp] == f.search_pp
        assert QUERIES[f.public.search_query][0] == f.search_query and f.op == f.public.search
