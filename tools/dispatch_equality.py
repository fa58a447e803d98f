"""Do two builds of libpybold_hip.so answer the dispatch queries alike?  No GPU is needed: the queries only decide.

    python tools/dispatch_equality.py <lib A> <lib B> [--jobs J]

Compared over a grid of call shapes (N scans, K taps, P problems, the three stop rules, four window lengths):
pb_fista_which_kernel (cost trace on and off), pb_fista_plan, pb_fista_plan_ex (seven flag sets), pb_fista_which_kernel_d,
pb_auto_lbda_supported, and pb_fista_list_plan over its three kinds.  Prints the number of answers compared and the first
difference, and exits with 1 if there is one."""
import argparse
import ctypes
import itertools
import multiprocessing
import sys

NS = list(range(1, 1401)) + [2000, 2432, 2433, 5000]
KS = [1, 8, 16, 27, 30, 32, 33, 34, 42, 48, 49, 64, 65, 66]
PS = [1, 2, 3, 1023, 1024, 2047, 2048, 4095, 4096, 4608, 4609, 5119, 5120, 8192, 8193, 10000, 12500, 16384, 20000, 100000]
STOPS = [0, 1, 2]
WINDS = [4, 5, 6, 8]
NO_MFMA, FORCE_PAIR, ONE_LAUNCH, ONE_STREAM, FORCE_MFMA2 = 8192, 8, 32, 128, 65536
FLAG_SETS = [0, NO_MFMA, FORCE_PAIR, ONE_LAUNCH, ONE_STREAM, FORCE_MFMA2, NO_MFMA | ONE_LAUNCH]
CANDS = 10                                   # plan.h: CAND_COUNT

_libs = None


def _load(paths):
    global _libs
    _libs = [ctypes.CDLL(p) for p in paths]


def _plan(lib, fn, *args):
    nm, mf, tf = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    rc = getattr(lib, fn)(*args, ctypes.byref(nm), ctypes.byref(mf), ctypes.byref(tf))
    return rc, nm.value, mf.value, tf.value


def _queries(lib, N):
    """Every answer of the shape-keyed queries for one series length, as (key, answer) pairs."""
    for K in KS:
        for stop, wind in itertools.product(STOPS, WINDS):
            yield ("which_kernel_d", N, K, stop, wind), lib.pb_fista_which_kernel_d(N, K, 0, stop, wind)
            for P in PS:
                for trace in (0, 1):
                    yield ("which_kernel", N, K, P, trace, stop, wind), lib.pb_fista_which_kernel(N, K, P, trace, stop, wind)
                yield ("plan", N, K, P, stop, wind), _plan(lib, "pb_fista_plan", N, K, P, stop, wind)
                for fl in FLAG_SETS:
                    yield ("plan_ex", N, K, P, stop, wind, fl), _plan(lib, "pb_fista_plan_ex", N, K, P, stop, wind, fl)
        for wind in WINDS:
            yield ("auto_lbda_supported", N, K, wind), lib.pb_auto_lbda_supported(N, K, wind)


def _list_plans(lib):
    """pb_fista_list_plan: the plan of a device-side list of n problems (kinds 1, 2) or of a partitioned call (kind 3)."""
    lens = sorted(set(PS + [0, 4607, 6144, 6145, 9216, 12288, 16383, 16385, 24576, 32768, 40000]))
    rg, bd = (ctypes.c_int32 * (2 * CANDS))(), (ctypes.c_int32 * CANDS)()
    for kind, n, pair, wide, one_stream, mfma2, chunks in itertools.product((1, 2, 3), lens, (0, 1), (0, 1), (0, 1), (0, 1), (1, 2)):
        for n_max in (n, n + 5000, 100000):
            if n_max < n:
                continue
            rc = lib.pb_fista_list_plan(kind, n, n_max, pair, wide, one_stream, mfma2, chunks, rg, bd)
            yield ("list_plan", kind, n, n_max, pair, wide, one_stream, mfma2, chunks), (rc, tuple(rg), tuple(bd))


def _compare(gen_a, gen_b):
    count, first = 0, None
    for (key, a), (_, b) in zip(gen_a, gen_b):
        count += 1
        if a != b and first is None:
            first = (key, a, b)
    return count, first


def _work(N):
    return _compare(_queries(_libs[0], N), _queries(_libs[1], N))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    _load(args.libs)
    total, first = _compare(_list_plans(_libs[0]), _list_plans(_libs[1]))
    with multiprocessing.Pool(args.jobs, initializer=_load, initargs=(args.libs,)) as pool:
        for count, diff in pool.imap(_work, NS, chunksize=4):
            total += count
            first = first or diff
    print("grid: %d series lengths (1..1400, 2000, 2432, 2433, 5000) x %d tap counts x %d problem counts x 3 stop rules x winds %s; "
          "plan_ex flag sets %s" % (len(NS), len(KS), len(PS), WINDS, FLAG_SETS))
    print("answers compared: %d" % total)
    print("first difference: %s" % ("none" if first is None else "%s: %s against %s" % first))
    sys.exit(0 if first is None else 1)
