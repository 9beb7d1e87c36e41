"""Case builders for the seams of the water-filling closed form (tests/test_gpu_fill_seams.py
runs them on the GPU, tests/test_fill_cases.py checks on the CPU that each one sits on the
seam it names).

The closed form: with c = max(free, 1) per live queued worker, S(r) = sum min(c, r), the fill
level L is the largest r with S(r) <= N (N = orphans + pending tasks), round L is served to
its first N - S(L) workers.  A round table of R rows is exact while L + 2 rows fit, even if a
worker holds more than R (`maxc > R && L >= R - 1` asks for a wider table); R comes from
choose_R of what the host can know at launch and saturates at ROW_LIMIT.

Every case has the same population: most live workers with c > L + 1 (so rounds L and L + 1
are both populated), a tenth with c in 1..3 (rows differ), about 5 % expired with in-flight
log entries (orphans, dispatched first), a queue over at least three 256-position blocks at
the default W, and T chosen so that round L is served to about a third of its workers.
"""
import numpy as np

from plan_cases import ROW_LIMIT, choose_R

EV_REGISTER, EV_RESULT = 0, 3
NOW, TTE = 1000.0, 10.0
INT32_MAX = (1 << 31) - 1
BLOCK = 256  # queue positions per queue block (kBS)


def water_fill(c, n):
    """The ten-line reference: (L, S(L), |A_L|, N_eff) of free counts c and n tasks."""
    c = np.asarray(c, np.int64)
    c = c[c > 0]
    n_eff = min(int(n), int(c.sum()))
    lo, hi = 0, int(c.max()) if len(c) else 0
    while lo < hi:  # S is monotone in r: the largest r with S(r) <= N_eff
        mid = (lo + hi + 1) // 2
        if int(np.minimum(c, mid).sum()) <= n_eff:
            lo = mid
        else:
            hi = mid - 1
    return lo, int(np.minimum(c, lo).sum()), int((c > lo).sum()), n_eff


def fill_case(L, cap0=None, maxc=None, way=None, batch="host", device_checked=True, n_wide=7, W=600, seed=0,
              expire=True, limit=ROW_LIMIT):
    """One tick that ends at fill level L.

    cap0: the largest free count of the loaded queue (default: the table that holds L + 2
    rows, choose_R(L + 2): the table is known at launch, maxc <= R).  The live workers that
    are not poor hold between min(L + 2, cap0) and cap0.
    maxc / way: n_wide live workers get `maxc` free processes -- "load": in the loaded state
    (the launch knows); "result": they are loaded with maxc - 1 and one result each raises
    them (the host never sees the count); "register": a register message with val = maxc
    (the host sees it only in a batch it checks itself: batch == "host", or a context whose
    batches the device does not check, device_checked False).
    expire False: nobody expires (deque contexts have no liveness).

    Returns dict(st, ev, T, log_cap, L, maxc, R_launch, reruns, erange): ev = (kind, slot, val,
    ts, seq); R_launch the table of the first launch, reruns whether the tick must rerun wider,
    erange whether it must fail with FB_ERANGE instead (L + 2 rows beyond the limit)."""
    assert way in (None, "load", "result", "register") and batch in ("host", "pinned", "device")
    rng = np.random.default_rng(seed * 100003 + L * 7 + (maxc or 0) % 9973)
    if cap0 is None:
        cap0 = choose_R(L + 2, 1 << 30)
    lo = min(L + 2, cap0)
    free = rng.integers(lo, cap0 + 1, W).astype(np.int64)
    free[0] = cap0  # the load's hint: the largest free count of the queue
    who = 1 + rng.permutation(W - 1)  # (worker 0 keeps cap0)
    poor, dead = np.zeros(W, bool), np.zeros(W, bool)
    poor[who[: max(2, W // 10)]] = True
    free[poor] = rng.integers(1, 4, int(poor.sum()))
    if expire:
        dead[who[-max(1, W // 20):]] = True
    hb = np.where(dead, 900.0, 999.0)
    log = rng.integers(0, W, 2 * W).astype(np.int32)
    if dead.any():
        log[:8] = np.nonzero(dead)[0][0]  # at least a few orphans
    rich = np.nonzero(~poor & ~dead)[0]
    rich = rich[rich != 0]
    wide = rng.choice(rich, n_wide, replace=False) if way else np.zeros(0, np.int64)
    wide.sort()
    ev = [np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.int64)]
    post = free.copy()
    vmax_known = 0
    if way == "load":
        free[wide] = post[wide] = maxc
    elif way == "result":
        assert maxc < INT32_MAX  # a result adds one: the count it raises stays an int32
        free[wide] = maxc - 1
        post[wide] = maxc
        seq = np.full(n_wide, -1, np.int64)
        for i, s in enumerate(wide[: n_wide // 2]):  # half of them complete an in-flight entry
            log[4 * W // 3 + i] = s
            seq[i] = 4 * W // 3 + i
        ev = [np.full(n_wide, EV_RESULT, np.uint8), wide.astype(np.int32), np.zeros(n_wide, np.int32),
              np.linspace(999.1, 999.9, n_wide), seq]
    elif way == "register":
        post[wide] = maxc
        ev = [np.full(n_wide, EV_REGISTER, np.uint8), wide.astype(np.int32), np.full(n_wide, maxc, np.int32),
              np.linspace(999.1, 999.9, n_wide), np.full(n_wide, -1, np.int64)]
        if batch == "host" or not device_checked:
            vmax_known = maxc
    queue = rng.permutation(W).astype(np.int32)
    st = dict(reg=np.ones(W, np.uint8), free=free.astype(np.int32), hb=hb, epoch=np.zeros(W, np.uint32),
              queue=queue, log=log)
    live_log = log.copy()
    if way == "result":
        live_log[ev[4][ev[4] >= 0]] = -1
    n_orph = int(dead[live_log[live_log >= 0]].sum())
    c = np.where(dead, 0, np.maximum(post, 1))
    S_L = int(np.minimum(c, L).sum())
    A_L = int((c > L).sum())
    T = S_L + A_L // 3 - n_orph
    assert T >= 0 and A_L > 0, (L, T, A_L)
    maxc_seen = int(c.max())
    R_launch = choose_R(max(int(free[queue].max()), vmax_known), limit)
    too_narrow = maxc_seen > R_launch and L >= R_launch - 1
    erange = maxc_seen > limit and L >= limit - 1
    return dict(st=st, ev=tuple(ev), T=T, log_cap=len(log) + T + n_orph + 64, L=L, maxc=maxc_seen, R_launch=R_launch,
                reruns=too_narrow and not erange, erange=erange, n_orph=n_orph, c=c, wide=wide)


def tick_args(case, now=NOW):
    """The positional arguments of GpuBalancer.tick / Oracle.tick for the case."""
    return (now, TTE) + tuple(case["ev"]) + (case["T"],)


# ---------------------------------------------------------------------------------------
# The cases, by the seam they sit on (the GPU tests parametrise over these lists)

# a. the table known at launch (maxc <= R): either side of 64, of the 128-row fused table
# (126 = R - 2 at R = 128), of the second and third 64-round register chunk (128, 190 / 191),
# of the compact form's byte and the 256-row table (253 .. 256), and wide tables
KNOWN_LEVELS = (63, 64, 125, 126, 127, 128, 129, 190, 191, 253, 254, 255, 256, 510, 1022)
DEQUE_LEVELS = (63, 126, 127, 191, 254, 1022)
# the smallest queue whose 128-row table is too large for the fused tick: nbq * 128 > kTabLd *
# kBS * 4 = 16384, i.e. more than 128 queue blocks
UNFUSED_W = 129 * BLOCK + 17


def known_case(L, W=600, expire=True):
    return fill_case(L, W=W, expire=expire, seed=1)


# b. a worker wider than the launch's table
WIDE_TABLES = (32, 64, 128)


def wide_levels(R):
    return (R - 3, R - 2, R - 1, R)


def wide_case(R, L, maxc, way, batch="host", device_checked=True):
    return fill_case(L, cap0=R, maxc=maxc, way=way, batch=batch, device_checked=device_checked, seed=2)


def wide_cases(way):
    """(R, L, maxc) of section b for one way of getting wider (a result adds exactly one)."""
    return [(R, L, m) for R in WIDE_TABLES for L in wide_levels(R) for m in ((R + 1,) if way == "result" else
                                                                             (R + 1, 4 * R))]


# d. the row limit: few workers (T is about W x limit)
LIMIT_MAXC = (ROW_LIMIT + 1, (1 << 30) + 1, INT32_MAX - 1)
LIMIT_W = 24


def limit_case(L, maxc, way):
    """way "load" or "register"; the other workers hold a little more than L + 1."""
    return fill_case(L, cap0=min(L + 6, maxc), maxc=maxc, way=way, n_wide=3, W=LIMIT_W, seed=3)


# e. sharded: the first launch has min(choose_R(hint), 128) rows, the relaunch choose_R(maxc)
SHARD_FIRST = [(R, m) for R in WIDE_TABLES for m in (R + 1, 255, 256, 70000) if m > R]
SHARD_WIDE_LEVELS = (63, 64, 65, 127, 128, 129, 4031, 4032, 4094)
SHARD_WIDE_MAXC = (65535, 65536, 70000)


def shard_case(L, R_first, maxc, W=600):
    """Loaded with the wide workers in the queue; the test states the first table with
    fb_set_round_hint(R_first), as a caller whose hint is stale would."""
    return fill_case(L, cap0=R_first if L <= R_first else L + 6, maxc=maxc, way="load", W=W, seed=4)
