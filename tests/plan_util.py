"""The kernel choice of the step and rollout paths, restated in Python: which instantiation the library launches for an (N, E)
batch.  The oracle tests enumerate it (tests/test_gpu_plan_oracle.py), and tests/test_plan_util.py pins it to the library's own
mdr::plan_step / mdr::plan_rollout through ctypes, so that a new branch of the planner shows up as a form without an oracle case.

Restated with the experiment knobs unset (MDR_PLAN_MULTI, MDR_PLAN_PACKED, MDR_PLAN_PACKED_FILL, MDR_PLAN_THREADS,
MDR_SPLIT_THREADS).  Forms are named as in the source, e.g. "k_step_group<16,4>", "k_rollout_fused<4,1,256,false,true>";
rocprof_name() gives the name a kernel trace prints."""

STEP_FUSED, STEP_GROUP, STEP_SPLIT, STEP_SINGLE, STEP_MULTI, STEP_PACKED = range(6)   # mdr_kernels.h:221

DEVICE_FILL = 262144            # E * N at which plan_step takes the device-filling branches
WINDOW_LANES = 64 * 8 * 256     # launch_rollout_fused: fewer lanes (or E * threads) than this run the WINDOW forms
MAX_N = 4096                    # reachable_forms() covers 1 <= N <= MAX_N
CONTROLLERS = ("bangbang", "deadband", "always_on")   # the in-kernel controllers; only bang-bang selects BB = true


def _pow2_at_least(n):
    g = 1
    while g < n:
        g <<= 1
    return g


def plan_step(N, E):
    """mdr_kernels.hip:2296-2367 (plan_step): (kind, vec, threads, tiles)."""
    vec = 4 if N % 4 == 0 else (2 if N % 2 == 0 else 1)
    if N <= 64 and E * N < DEVICE_FILL:
        vec = 1
    lanes = (N + vec - 1) // vec
    if N % 4 == 2 and 6 <= N <= 126 and E >= 2 and E * N >= DEVICE_FILL:
        return (STEP_MULTI, 4, _pow2_at_least(N // 2), 2)
    if N % 4 == 0 and 12 <= N <= 128 and E * N >= DEVICE_FILL:
        L = N // 4
        per_wave = 64 // L
        if (L & (L - 1)) != 0 and 1000 * L < 650 * _pow2_at_least(L) and per_wave * _pow2_at_least(L) > 64:
            return (STEP_PACKED, 4, L, per_wave)
    if N == 1 and E % 4 == 0 and E >= DEVICE_FILL:
        return (STEP_SINGLE, 4, 256, 1)
    if lanes <= 32 or (vec < 4 and lanes <= 64):
        return (STEP_GROUP, vec, _pow2_at_least(lanes), 1)
    if N % 4 == 0 and N <= 4096:
        threads = 64 if N <= 256 else (128 if N <= 512 else 256)
        return (STEP_FUSED, 4, threads, (N + threads * 4 - 1) // (threads * 4))
    if N <= 1024:
        return (STEP_FUSED, 1, 256, (N + 255) // 256)
    return (STEP_SPLIT, 4 if N % 4 == 0 else 1, 256, 1)


def plan_rollout(N, E):
    """mdr_kernels.hip:2370-2397 (plan_rollout): (kind, vec, threads, tiles)."""
    kind, vec, threads, tiles = plan_step(N, E)
    if kind in (STEP_GROUP, STEP_PACKED):
        return (kind, vec, threads, tiles)
    if kind == STEP_MULTI:
        return (STEP_GROUP, 2, threads, 1)
    if kind == STEP_SINGLE:
        return (STEP_GROUP, 1, 1, tiles)
    if N % 4 == 0 and N <= 2048:
        threads = 64 if N <= 256 else (128 if N <= 512 else 256)
        return (STEP_FUSED, 4, threads, (N + threads * 4 - 1) // (threads * 4))
    if N <= 512:
        return (STEP_FUSED, 1, 256, (N + 255) // 256)
    return (STEP_SPLIT, 0, 0, 0)


def _b(x):
    return "true" if x else "false"


def step_kernel(N, E):
    """The instantiation launch_step starts for one step (mdr_kernels.hip:2535-2583).  launch_fused_tiles
    (mdr_kernels.hip:2279-2288) maps tiles 1, 2, 3 and anything else to 4; launch_step_multi (mdr_multi.hip:359-375) takes
    k_step_packed or k_step_multi<threads>; the split path (launch_step_begin_split / launch_step_end_split,
    mdr_kernels.hip:2420-2445, MDR_SPLIT_THREADS unset) is two launches, named "partial+finish"."""
    kind, vec, threads, tiles = plan_step(N, E)
    if kind == STEP_PACKED:
        return "k_step_packed"
    if kind == STEP_MULTI:
        return "k_step_multi<%d>" % threads
    if kind == STEP_SINGLE:
        return "k_step_single_house"
    if kind == STEP_FUSED:
        t = min(tiles, 4)
        return "k_step_fused<%d,%d,%d>" % ((4, t, threads) if vec == 4 else (1, t, 256))
    if kind == STEP_GROUP:
        return "k_step_group<%d,%d>" % (min(threads, 64), vec)
    v = 1 if N % 4 != 0 else 4
    return "k_step_partial<%d,256>+k_step_finish<%d,256>" % (v, v)


def rollout_kernel(N, E, controller="bangbang"):
    """The instantiation mdr_env_rollout_fused launches (launch_rollout_fused, mdr_kernels.hip:2449-2510; STEP_PACKED through
    launch_rollout_multi, mdr_multi.hip:372-379), or None where the rollout plan has no multi-step kernel (STEP_SPLIT): the library
    then runs step_kernel(N, E) once per step (mdr_api.hip, mdr_env_rollout_fused)."""
    if controller not in CONTROLLERS:
        raise ValueError(controller)
    bb = controller == "bangbang"
    kind, vec, threads, tiles = plan_rollout(N, E)
    if kind == STEP_PACKED:
        return "k_rollout_packed<%s>" % _b(bb)
    if kind == STEP_GROUP:
        win = E * threads < WINDOW_LANES
        return "k_rollout_group<%d,%d,%s,%s>" % (min(threads, 64), vec, _b(win), _b(bb))
    if kind == STEP_FUSED:
        win = E * threads < WINDOW_LANES
        if vec == 4:
            th = threads if threads in (64, 128) else 256
            return "k_rollout_fused<4,%d,%d,%s,%s>" % (1 if tiles == 1 else 2, th, _b(win), _b(bb))
        return "k_rollout_fused<1,%d,256,%s,%s>" % (1 if tiles == 1 else 2, _b(win), _b(bb))
    return None


def critical_envs(N):
    """Every E at which the plans for N change, with its neighbours: between two of these the forms are constant in E."""
    es = {1, 2, 3, 4, 5}
    e0 = -(-DEVICE_FILL // N)
    es.update((e0 - 1, e0, e0 + 1))
    for t in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        w = -(-WINDOW_LANES // t)
        es.update((w - 1, w, w + 1))
    if N == 1:
        es.update((DEVICE_FILL, DEVICE_FILL + 1, DEVICE_FILL + 3, DEVICE_FILL + 4))
    return sorted(e for e in es if e >= 1)


def forms_of(N, E):
    """Every form a batch of this size can launch: the step form and the rollout form under each controller."""
    out = {step_kernel(N, E)}
    for c in CONTROLLERS:
        r = rollout_kernel(N, E, c)
        if r is not None:
            out.add(r)
    return out


def reachable_forms():
    """Every step and rollout instantiation the launch functions reach for 1 <= N <= 4096 (any E >= 1, knobs unset)."""
    out = set()
    for N in range(1, MAX_N + 1):
        for E in critical_envs(N):
            out |= forms_of(N, E)
    return out


def oracle_cases():
    """One (form, N, E, controller) case per reachable form: the smallest batch (fewest houses, then fewest houses per env) that
    launches it.  E is made odd where E + 1 still selects the form, so the last wavefront / group / packed wave is part-filled.
    `controller` is the one that selects the form (None for a step form)."""
    best = {}
    for N in range(1, MAX_N + 1):
        for E in critical_envs(N):
            key = (E * N, N, E)
            cands = [(step_kernel(N, E), None)] + [(rollout_kernel(N, E, c), c) for c in ("bangbang", "deadband")]
            for form, ctl in cands:
                if form is not None and (form not in best or key < best[form][0]):
                    best[form] = (key, ctl)
    cases = []
    for form in sorted(best):
        (_, N, E), ctl = best[form]
        kernel = (lambda n, e: step_kernel(n, e)) if ctl is None else (lambda n, e: rollout_kernel(n, e, ctl))
        if E % 2 == 0 and kernel(N, E + 1) == form:
            E += 1
        cases.append((form, N, E, ctl))
    return cases


def case_forms(N, E, controller):
    """The form a case is meant for, as oracle_cases() decides it."""
    return step_kernel(N, E) if controller is None else rollout_kernel(N, E, controller)


def launched_kernels(form):
    """The kernel launches behind a form name (the split step is two)."""
    return form.split("+")


def rocprof_name(kernel):
    """The name a kernel trace prints, without the argument list: "k_step_group<16,4>" -> "mdr::k_step_group<16, 4>"."""
    return "mdr::" + kernel.replace(",", ", ")
