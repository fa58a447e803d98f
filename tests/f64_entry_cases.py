"""The calls and query points behind tests/golden/f64_entry_errors.json: what the twelve float64 register-family entry points
(pb_fista_solve_d, pb_fista_solve_pp_d, the two pb_fista_solve_split_long*_d and the eight pb_auto_lbda*_d) answer to a call
they refuse, and what the family's queries answer on a grid around every limit.  A plain helper module: the recorder
(tests/golden/make_f64_entry_errors.py) and the replay (tests/test_f64_entry_errors_host.py) both build their calls here.

No case may pass validation with a positive count: the device pointers are not memory.  Every case therefore carries one
fault at least, or P == 0 / V == 0 -- asserted where the cases are built; a call shape that is NOT a fault on its own (another
form, the LDS kernel) is a `variant` and is only ever recorded beside a fault or a zero count."""
import ctypes
import hashlib
import itertools

NONE, LOOPS, WINDOW = 0, 1, 2
GENERIC, FAST, PP_SPLIT, LONG_HRF = 1, 2, 1048576, 2097152
FAKE, HOST = "fake", "host"          # a device pointer that is never read; a real host buffer (taps_host is read before a launch)
MANY = (1 << 25) + 1

FORMS = {                            # name: (first scan count, last, tap limit, base N, base K)
    "one_wave": (1, 640, 32, 300, 30),
    "four_waves": (641, 1280, 32, 1200, 30),
    "long": (1, 640, 48, 300, 42),
    "four_waves_long": (641, 1280, 48, 1200, 42),
}

SOLVE_ARGS = ("y", "ldy", "y_rep", "w", "ldw", "P", "N", "taps_host", "taps_dev", "K", "step", "lbda", "lbda_dev", "betas",
              "n_iter", "J", "ldj", "stop", "tol", "wind", "n_done", "flags", "stream")
SOLVE_PP_ARGS = ("y", "ldy", "y_rep", "w", "ldw", "P", "N", "taps_dev", "ldt", "K", "step_dev", "lbda", "lbda_dev", "betas",
                 "n_iter", "J", "ldj", "stop", "tol", "wind", "n_done", "flags", "stream")
SEARCH_ARGS = ("y", "ldy", "w", "ldw", "cold", "V", "N", "taps_host", "K", "step", "betas", "sigma", "early", "tol", "wind",
               "nb_iter", "nb_sub_iter", "chunk", "R", "G", "J", "ldtr", "alpha", "lbda_out", "n_outer", "n_inner", "work",
               "work_len", "stream")
SEARCH_PP_ARGS = ("y", "ldy", "w", "ldw", "cold", "V", "N", "taps_dev", "ldt", "K", "step_dev", "betas", "sigma", "early", "tol",
                  "wind", "nb_iter", "nb_sub_iter", "chunk", "R", "G", "J", "ldtr", "alpha", "lbda_out", "n_outer", "n_inner",
                  "work", "work_len", "stream")
ARGS = {"solve": SOLVE_ARGS, "solve_pp": SOLVE_PP_ARGS, "search": SEARCH_ARGS, "search_pp": SEARCH_PP_ARGS}


def base_args(kind, N, K, flags=0):
    pp = kind.endswith("_pp")
    if kind.startswith("solve"):
        a = dict(y=FAKE, ldy="N", y_rep=1, w=FAKE, ldw="N", P=3, N=N, K=K, lbda=1.0, lbda_dev=None, betas=FAKE, n_iter=10,
                 J=None, ldj=0, stop=NONE, tol=0.0, wind=6, n_done=FAKE, flags=flags, stream=None)
        a.update(dict(taps_dev=FAKE, ldt="K", step_dev=FAKE) if pp else dict(taps_host=HOST, taps_dev=FAKE, step=1.0))
    else:
        a = dict(y=FAKE, ldy="N", w=FAKE, ldw="N", cold=1, V=3, N=N, K=K, betas=FAKE, sigma=FAKE, early=1, tol=1e-6, wind=6,
                 nb_iter=10, nb_sub_iter=10, chunk=0, R=None, G=None, J=None, ldtr=0, alpha=FAKE, lbda_out=FAKE, n_outer=FAKE,
                 n_inner=FAKE, work=FAKE, work_len="need", stream=None)
        a.update(dict(taps_dev=FAKE, ldt="K", step_dev=FAKE) if pp else dict(taps_host=HOST, step=1.0))
    return a


def solve_faults(pp):
    """Single faults of every solve family: one per check of the validation order that no form owns."""
    f = [dict(P=-1), dict(N=0), dict(K=0), dict(n_iter=-1), dict(y_rep=0)]
    f += [dict(ldt="K-1")] if pp else []
    f += [dict(ldy="N-1"), dict(ldw="N-1"), dict(J=FAKE, ldj="n_iter-1")]
    f += [] if pp else [dict(step=0.0)]
    f += [dict(stop=-1), dict(stop=3), dict(stop=WINDOW, wind=1), dict(y=None), dict(w=None), dict(betas=None)]
    f += [dict(taps_dev=None), dict(step_dev=None)] if pp else []
    return f + [dict(P=MANY)]


def search_faults(pp, n_lo, n_hi, k_max):
    f = [dict(V=-1), dict(N=0), dict(K=0), dict(wind=4)]
    f += [dict(N=n_lo - 1)] if n_lo > 1 else []
    f += [dict(N=n_hi + 1), dict(K=k_max + 1), dict(nb_iter=0), dict(nb_sub_iter=-1), dict(chunk=-1), dict(ldy="N-1"),
          dict(ldw="N-1")]
    f += [dict(ldt="K-1")] if pp else []
    f += [dict(R=FAKE, ldtr="nb_iter-1"), dict(G=FAKE, ldtr="nb_iter-1"), dict(J=FAKE, ldtr="nb_iter-1")]
    f += [] if pp else [dict(step=0.0)]
    f += [dict(work_len="need-1"), dict(y=None), dict(w=None), dict(taps_dev=None) if pp else dict(taps_host=None)]
    f += [dict(step_dev=None)] if pp else []
    return f + [dict(sigma=None), dict(work=None), dict(betas=None), dict(V=MANY)]


def named_form_faults(n_lo, n_hi, k_max, excluded):
    f = [dict(N=n_lo - 1)] if n_lo > 1 else []
    return f + [dict(N=n_hi + 1), dict(K=k_max + 1), dict(stop=WINDOW, wind=4)] + [dict(flags_or=x) for x in excluded]


def families():
    """name -> (entry point, kind, base arguments, faults, variants): the sixteen form x kind families, and the default
    dispatch of pb_fista_solve_d / pb_fista_solve_pp_d."""
    fam = {}
    for form, (n_lo, n_hi, k_max, N, K) in FORMS.items():
        tag = {"one_wave": "", "four_waves": "_split", "long": "_long", "four_waves_long": "_split_long"}[form]
        for pp in (False, True):
            kind = "search_pp" if pp else "search"
            fam["%s/%s" % (form, kind)] = ("pb_auto_lbda%s%s_d" % (tag, "_pp" if pp else ""), kind, base_args(kind, N, K),
                                            search_faults(pp, n_lo, n_hi, k_max), [dict(alpha=None, lbda_out=None), dict(early=0)])
    spare_host = [dict(taps_dev=None)]               # the register forms read taps_host only
    # one wave: PB_FLAG_FORCE_FAST is "the one-wave form or an error"
    fam["one_wave/solve"] = ("pb_fista_solve_d", "solve", base_args("solve", 300, 30, FAST),
                             solve_faults(False) + [dict(N=641), dict(K=33), dict(stop=WINDOW, wind=4), dict(flags_or=GENERIC),
                                                    dict(flags_or=LONG_HRF), dict(taps_host=None)],
                             spare_host + [dict(flags_or=PP_SPLIT)])
    fam["one_wave/solve_pp"] = ("pb_fista_solve_pp_d", "solve_pp", base_args("solve_pp", 300, 30, FAST),
                                solve_faults(True) + [dict(N=641), dict(K=33), dict(stop=WINDOW, wind=4), dict(flags_or=GENERIC),
                                                      dict(flags_or=LONG_HRF), dict(flags_or=PP_SPLIT)], [])
    # four waves, taps on the host: reached by the dispatch of pb_fista_solve_d only -- leaving its shapes is no fault
    fam["four_waves/solve"] = ("pb_fista_solve_d", "solve", base_args("solve", 1200, 30),
                               # (the two flags are faults AT these scan counts: they name their N, so no variant's N replaces it)
                               solve_faults(False) + [dict(flags_or=FAST, N=1200), dict(flags_or=LONG_HRF, N=1200), dict(N=100000)],
                               spare_host + [dict(N=640), dict(N=1281), dict(K=33), dict(stop=WINDOW, wind=4), dict(flags_or=GENERIC),
                                             dict(taps_host=None), dict(flags_or=PP_SPLIT)])
    fam["four_waves/solve_pp"] = ("pb_fista_solve_pp_d", "solve_pp", base_args("solve_pp", 1200, 30, PP_SPLIT),
                                  solve_faults(True) + named_form_faults(641, 1280, 32, (GENERIC, FAST, LONG_HRF)), [])
    fam["long/solve"] = ("pb_fista_solve_d", "solve", base_args("solve", 300, 42, LONG_HRF),
                         solve_faults(False) + named_form_faults(1, 640, 48, (GENERIC, FAST, PP_SPLIT)) + [dict(taps_host=None)],
                         spare_host)
    fam["long/solve_pp"] = ("pb_fista_solve_pp_d", "solve_pp", base_args("solve_pp", 300, 42, LONG_HRF),
                            solve_faults(True) + named_form_faults(1, 640, 48, (GENERIC, FAST, PP_SPLIT)), [])
    fam["four_waves_long/solve"] = ("pb_fista_solve_split_long_d", "solve", base_args("solve", 1200, 42),
                                    solve_faults(False) + named_form_faults(641, 1280, 48, (GENERIC, FAST, PP_SPLIT, LONG_HRF))
                                    + [dict(taps_host=None)], spare_host)
    fam["four_waves_long/solve_pp"] = ("pb_fista_solve_split_long_pp_d", "solve_pp", base_args("solve_pp", 1200, 42),
                                       solve_faults(True) + named_form_faults(641, 1280, 48, (GENERIC, FAST, PP_SPLIT, LONG_HRF)), [])
    # the default dispatch: one wave, else four (taps on the host only), else the LDS kernel
    beyond = [dict(N=700, flags_or=FAST), dict(N=1300, flags_or=FAST), dict(K=33, flags_or=FAST), dict(N=100000)]
    shapes = [dict(flags_or=GENERIC), dict(flags_or=FAST), dict(N=700), dict(N=1300), dict(K=33), dict(stop=WINDOW, wind=4)]
    fam["default/solve"] = ("pb_fista_solve_d", "solve", base_args("solve", 300, 30), solve_faults(False) + beyond,
                            spare_host + shapes + [dict(taps_host=None), dict(flags_or=PP_SPLIT)])
    fam["default/solve_pp"] = ("pb_fista_solve_pp_d", "solve_pp", base_args("solve_pp", 300, 30), solve_faults(True) + beyond, shapes)
    assert len(fam) == 18
    return fam


def merged(*parts):
    """One override from several, or None when two of them set the same argument (flags are or-ed)."""
    out = {}
    for p in parts:
        for k, v in p.items():
            if k == "flags_or":
                out[k] = out.get(k, 0) | v
            elif k in out and out[k] != v:
                return None
            else:
                out[k] = v
    return out


def cases():
    """[(family, override)], in a fixed order: every single fault, every pair of faults, every fault beside every variant, and
    the zero count alone, beside every fault and beside every variant."""
    out = []
    for name, (entry, kind, base, faults, variants) in families().items():
        zero = dict(P=0) if kind.startswith("solve") else dict(V=0)
        todo = [merged(f) for f in faults]
        todo += [merged(a, b) for a, b in itertools.combinations(faults, 2)]
        todo += [merged(f, v) for f in faults for v in variants]
        carries = len(todo)                                   # up to here: a fault in every case
        todo += [zero] + [merged(x, zero) for x in faults + variants]
        for i, over in enumerate(todo):
            if over is None:
                continue
            assert i < carries or over.get("P", over.get("V")) == 0, (name, over)
            out.append((name, over))
    return out


def case_list_hash():
    text = repr([(n, sorted(o.items())) for n, o in cases()]) + repr(sorted((k, repr(v)) for k, v in families().items()))
    return hashlib.sha256(text.encode()).hexdigest()


def resolve(base, over):
    a = dict(base)
    a["flags"] = a.get("flags", 0) | over.get("flags_or", 0)
    a.update((k, v) for k, v in over.items() if k != "flags_or")
    count = a.get("V", 0)
    names = dict(N=a["N"], K=a["K"], n_iter=a.get("n_iter"), nb_iter=a.get("nb_iter"), need=12 * max(count, 0))
    for k, v in a.items():
        if isinstance(v, str) and v not in (FAKE, HOST):
            ref, minus = (v[:-2], 1) if v.endswith("-1") else (v, 0)
            a[k] = names[ref] - minus
    return a


_taps_host = (ctypes.c_double * 64)(*([1.0] * 64))


def call(lib, entry, kind, base, over):
    """(return code, pb_last_error() as text)."""
    a = resolve(base, over)
    ptr = {FAKE: ctypes.c_void_p(4096), HOST: ctypes.cast(_taps_host, ctypes.c_void_p)}
    if "flags" not in ARGS[kind]:
        a.pop("flags")
    vals = [ptr.get(a[k], a[k]) if isinstance(a[k], str) else a[k] for k in ARGS[kind]]
    rc = getattr(lib, entry)(*vals)
    count = a["P"] if kind.startswith("solve") else a["V"]
    return rc, lib.pb_last_error().decode(), count


def bind(path):
    """The library at `path` with the signatures of pybold_amd/_lib.py."""
    from pybold_amd import _lib
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def record_faults(lib):
    """{"messages": [[rc, text]], "results": {family: [index into messages]}}; the entry point's name at the head of a message
    is written "@" (entry 0: PB_OK, whose message is not recorded).  Refuses a case that passes validation with a count."""
    fam = families()
    table, index, results = [[0, ""]], {(0, ""): 0}, {}
    for name, over in cases():
        entry, kind, base = fam[name][:3]
        rc, msg, count = call(lib, entry, kind, base, over)
        # PB_ERR_INVALID, or the no-op: any other code means the call went past its validation towards a launch
        assert rc == -1 or (rc == 0 and count == 0), "%s %r passes validation with %d problems (%d, %s)" % (name, over, count, rc, msg)
        if msg.startswith(entry + ":"):
            msg = "@" + msg[len(entry):]
        key = (rc, "" if rc == 0 else msg)
        if key not in index:
            index[key] = len(table)
            table.append(list(key))
        results.setdefault(name, []).append(index[key])
    return {"messages": table, "results": results}


GRID_N = (-1, 0, 1, 2, 319, 320, 321, 322, 639, 640, 641, 642, 959, 960, 961, 962, 1279, 1280, 1281, 1282, 2000, 7000, 100000)
GRID_K = (-1, 0, 1, 2, 31, 32, 33, 34, 47, 48, 49, 50, 64, 65)
GRID_STOP = (-1, 0, 1, 2, 3)
GRID_WIND = (2, 4, 5, 6, 8)
GRID_V = (-1, 0, 1, 2, 600, 1 << 25, MANY, 2 ** 31 - 1)
QUERIES_4 = ("pb_fista_long_hrf_supported", "pb_fista_split_long_hrf_supported", "pb_fista_pp_split_supported")
QUERIES_WHICH = ("pb_fista_which_kernel_d", "pb_fista_which_kernel_pp_d")        # (N, K, with_cost_trace, stop_mode, wind)
QUERIES_3 = ("pb_auto_lbda_supported", "pb_auto_lbda_split_supported", "pb_auto_lbda_long_supported",
             "pb_auto_lbda_split_long_supported")


def _char(v):
    assert -1 <= v <= 9
    return "-" if v < 0 else str(v)


def query_block(lib, name, N, K):
    """The answers of one query at (N, K), one character each: over stop_mode x wind (with and without a cost trace for
    the two which_kernel queries), or over wind."""
    fn = getattr(lib, name)
    if name in QUERIES_3:
        return "".join(_char(fn(N, K, w)) for w in GRID_WIND)
    if name in QUERIES_WHICH:
        return "".join(_char(fn(N, K, wj, s, w)) for wj in (0, 1) for s in GRID_STOP for w in GRID_WIND)
    return "".join(_char(fn(N, K, s, w)) for s in GRID_STOP for w in GRID_WIND)


def record_queries(lib):
    """{query: {"blocks": [distinct blocks], "at": [index of the block at each (N, K), N-major]}}, and pb_auto_lbda_work_len."""
    out = {}
    for name in QUERIES_4 + QUERIES_WHICH + QUERIES_3:
        blocks, at = [], []
        for N in GRID_N:
            for K in GRID_K:
                b = query_block(lib, name, N, K)
                if b not in blocks:
                    blocks.append(b)
                at.append(blocks.index(b))
        out[name] = {"blocks": blocks, "at": at}
    out["pb_auto_lbda_work_len"] = [lib.pb_auto_lbda_work_len(V) for V in GRID_V]
    return out


def record(lib):
    return {"case_list_sha256": case_list_hash(), "faults": record_faults(lib), "queries": record_queries(lib)}
