"""The kernel choice of the fused actor, restated in Python: which instantiation mdr_actor_sample (observation rows or feature
planes) and mdr::launch_actor_observe (observe -> act) start for a shape, with how many waves per workgroup, or the status they
refuse it with (csrc/mdr_policy.hip).  tests/test_actor_forms.py holds the restatement to the instantiations compiled into
libmdr_hip.so and to the case table of tests/test_gpu_actor_forms.py; the style is that of tests/plan_util.py.

Restated with the experiment knobs unset (MDR_OBSERVE_GEN, MDR_OBSERVE_EXT) and the default build (MDR_WAVES16 = MDR_WAVES16_EXT =
16).  Forms carry every template argument, defaults included, as a kernel trace and the symbol table print them, without the
blanks: "k_actor_sample16<7,false,16>", "k_actor_observe16<7,true,true,false,13,true>"."""

FRAG32, FRAG16, BF16X3, FRAG16T = 0, 1, 2, 3                 # mdr_actor_layout
INVALID, UNSUPPORTED = -1, -4                                # MDR_ERR_INVALID, MDR_ERR_UNSUPPORTED
MAX_HIDDEN = 127
WAVES, WAVES16, WAVES16_EXT, WAVESB, NCB = 8, 16, 16, 8, 2
OBS_C, OBS_ROW, OBS_PAD, OBS_MAX_C = 10, 56, 16, 13
LDS_LIMIT = 160 * 1024
STATE_COLUMNS = {"hour": 2, "day": 2, "solar_gain": 1, "thermal": 5, "hvac": 2}      # floats each optional state flag adds


def _b(x):
    return "true" if x else "false"


def _acc_row_half0(q):
    return 32 * (q >> 4) + (q & 3) + 8 * ((q >> 2) & 3)


def blocks16(h1, h2):
    return 7 if max(h1, h2) <= 112 else 8


def steps1(layout, F):
    if layout == BF16X3:
        return (F + 31) // 32
    return (F + 3) // 4 if layout in (FRAG16, FRAG16T) else (F + 2) // 2


def steps1_order(layout, F, order):
    s = steps1(layout, F)
    if order != 1 or layout not in (FRAG16, FRAG16T) or s > 16:
        return s
    return 13 if s <= 13 else (15 if s <= 15 else 16)


def steps2(layout, h1):
    if layout == BF16X3:
        return 4
    if layout in (FRAG16, FRAG16T):
        return 4 * (h1 // 16) + (h1 % 16 + 3) // 4
    return sum(1 for q in range(64) if _acc_row_half0(q) <= h1)


def floats_per_step(layout):
    return 4096 if layout == BF16X3 else (512 if layout in (FRAG16, FRAG16T) else 256)


def tail_shape_ok(h1, h2):
    return h1 // 16 == 6 and h2 // 16 == 6 and 1 <= h1 % 16 <= 4 and 1 <= h2 % 16 <= 4


def rows_slices(F, A, plane_stride=0):
    """The (first agent, count) launches of the 16-agent fp32 forms: 32-bit byte offsets, so at most 4 GiB of rows per launch."""
    per = A if plane_stride else ((0xFFFFFFFF // (F * 4)) & ~15)
    return [(first, min(per, A - first)) for first in range(0, A, per)]


def select_rows(layout, F, H1, H2, A=1, plane_stride=0, feature_order=0):
    """mdr_actor_sample: (form, waves per workgroup) or the status code of the refusal."""
    if A < 0 or (plane_stride != 0 and plane_stride < A) or layout not in (FRAG32, FRAG16, BF16X3, FRAG16T):
        return INVALID
    if F <= 0 or H1 <= 0 or H2 <= 0 or feature_order != 0:
        return INVALID
    if H1 > MAX_HIDDEN or H2 > MAX_HIDDEN:
        return UNSUPPORTED
    lbf = layout == BF16X3
    l16 = layout in (FRAG16, FRAG16T) or lbf
    if layout == FRAG16T and not tail_shape_ok(H1, H2):
        return UNSUPPORTED
    if l16 and F > 128:
        return UNSUPPORTED
    s1, s2 = steps1(layout, F), steps2(layout, H1)
    if ((s1 + s2) * floats_per_step(layout) + 512) * 4 > LDS_LIMIT:
        return UNSUPPORTED
    mb = blocks16(H1, H2)
    if lbf:
        return ("k_actor_sample_bf16<%d,%d>" % (mb, 16 if s1 <= 2 else 32), WAVESB)
    if l16:
        if plane_stride != 0 and ((F - 1) * plane_stride + A) * 4 > 0xFFFFFFFF:
            return UNSUPPORTED
        tail = layout == FRAG16T
        return ("k_actor_sample16<%d,%s,%d>" % (7 if tail else mb, _b(tail), 16 if s1 <= 16 else 32), WAVES16)
    if s1 <= 32 and s2 == 52:
        return ("k_actor_sample<32,52>", WAVES)
    return ("k_actor_sample<%d,0>" % (32 if s1 <= 32 else 0), WAVES)


def observe_window_lanes(N, c, tile):
    worst = 0
    for h0 in range(N if N < 4096 else 1):
        lanes, hs, rem = 0, h0, tile
        while rem > 0:
            ln = min(N - hs, rem)
            lanes += N if ln + c >= N else ln + c
            rem -= ln
            hs = 0
        worst = max(worst, lanes)
    return tile + 2 * c if N >= 4096 else worst


def observe_shape(flags=(), nb_comm=10, defects=0.0, table=False):
    """What mdr_api.hip (actor_sample_impl) hands to launch_actor_observe for an observation: (ext, c, own)."""
    own = 11 + sum(STATE_COLUMNS[f] for f in flags)
    ext = bool(flags) or nb_comm != 10 or defects > 0.0 or table
    return ext, nb_comm, own


def select_observe(layout, H1, H2, N, E=1, ext=False, c=10, own=11, table=False, rows_out=False, feature_order=1, num_state=None,
                   msg_floats=None):
    """mdr::launch_actor_observe: (form, waves per workgroup) or the status code of the refusal.  `table`: senders through a link
    table (static or random_sample) instead of the circular neighbours; `num_state` / `msg_floats`: what the actor was packed for
    (default: this observation)."""
    if layout not in (FRAG16, BF16X3, FRAG16T):
        return UNSUPPORTED
    if layout == FRAG16T and not tail_shape_ok(H1, H2):
        return UNSUPPORTED
    if not ext:
        c, own = OBS_C, 11
    F = 4 * c + own
    num_state = F if num_state is None else num_state
    msg_floats = 4 * c if msg_floats is None else msg_floats
    if feature_order != 1 or num_state != F or msg_floats != 4 * c:
        return UNSUPPORTED
    if F > 64 or c > OBS_MAX_C or c < 0:
        return UNSUPPORTED
    if H1 <= 0 or H2 <= 0 or H1 > MAX_HIDDEN or H2 > MAX_HIDDEN:
        return INVALID
    lbf = layout == BF16X3
    tile = 16 * NCB if lbf else 16
    s1 = steps1_order(layout, F, feature_order)
    extk = 0 if (not ext or lbf) else s1
    row = OBS_ROW
    if ext:
        row = ((F if lbf else 4 * extk) + 2 + 3) & ~3
        if row & 4 == 0:
            row += 4
    waves = WAVESB if lbf else (WAVES16_EXT if ext else WAVES16)
    if N < c + 1:
        return UNSUPPORTED
    table = ext and table
    gen = N % 32 != 0 or table
    if gen and observe_window_lanes(N, 0 if table else c, tile) > 64:
        return UNSUPPORTED
    A = E * N
    if (A + tile - 1) // tile > 0x7FFFFFFF or (ext and A > 0x3FFFFFFF):
        return UNSUPPORTED
    s2 = steps2(layout, H1)
    mb = blocks16(H1, H2)
    window = tile * row + (max(64 - row, OBS_PAD) if lbf else OBS_PAD)

    def lds_need(w):
        s1_lds = (2 if lbf else extk) if ext else s1
        per_step = floats_per_step(layout)
        if ext and lbf:
            per_step = per_step * mb // 8
        return ((s1_lds + s2) * per_step + 512 + w * window) * 4 + (tile * F * 2 if rows_out else 0)

    if ext and lbf:
        while waves > 4 and lds_need(waves) > LDS_LIMIT:
            waves -= 1
    if ext and not lbf:
        while waves > 8 and lds_need(waves) > LDS_LIMIT:
            waves -= 4
    if lds_need(waves) > LDS_LIMIT:
        return UNSUPPORTED
    if lbf:
        return ("k_actor_observe_bf16<%d,%s,%s,%s,%s>" % (mb, _b(rows_out), _b(gen or table), _b(ext), _b(table)), waves)
    tail = layout == FRAG16T
    if ext:
        if extk not in (13, 15, 16):
            return UNSUPPORTED
        g = True if (table or not tail) else gen      # without the 4x4 tail the extended fp32 form always takes the general windows
        return ("k_actor_observe16<%d,%s,%s,%s,%d,%s>" % (7 if tail else mb, _b(rows_out), _b(g), _b(tail), extk, _b(table)), waves)
    return ("k_actor_observe16<%d,%s,%s,%s,0,false>" % (7 if tail else mb, _b(rows_out), _b(gen), _b(tail)), waves)


def family(form):
    """The kernel template a form instantiates: "k_actor_sample16<7,true,32>" -> "k_actor_sample16"."""
    return form.split("<")[0]


def reachable_forms():
    """Every instantiation the two launch functions reach, found by running the restated selection over the shapes that move it:
    layouts, hidden sizes on both sides of the 112-unit block edge, feature counts across every k-step edge, cluster sizes that do
    and do not take the general staging, every observation shape class, with and without rows_out."""
    out = set()
    hidden = [(100, 100), (112, 112), (113, 64), (64, 113), (127, 127), (64, 32), (97, 99), (1, 1)]
    for layout in (FRAG32, FRAG16, BF16X3, FRAG16T):
        for h1, h2 in hidden:
            for F in (1, 11, 51, 62, 63, 64, 65, 100, 128, 133, 180):
                r = select_rows(layout, F, h1, h2)
                if isinstance(r, tuple):
                    out.add(r[0])
            for flags, c in (((), 10), (("thermal", "hvac"), 10), (tuple(STATE_COLUMNS), 10), (("solar_gain",), 6), ((), 0), (("solar_gain",), 13)):
                for defects in (0.0, 0.1):
                    for table in (False, True):
                        ext, cc, own = observe_shape(flags, c, defects, table)
                        for N in (20, 50, 64, 1024, 4100):
                            for store in (False, True):
                                r = select_observe(layout, h1, h2, N, 3, ext, cc, own, table, store)
                                if isinstance(r, tuple):
                                    out.add(r[0])
    return out


def trace_name(form):
    """The name a kernel trace prints, without the argument list: "(anonymous namespace)::k_actor_sample16<7, false, 16>"."""
    return "(anonymous namespace)::" + form.replace(",", ", ")


def compiled_forms(library, readelf):
    """The k_actor_* instantiations in the host image of the built library: the kernel handles of its symbol table, demangled by
    the toolchain's llvm-readelf, written as this module writes forms."""
    import re
    import subprocess
    text = subprocess.run([readelf, "-sW", "--demangle", library], check=True, capture_output=True, text=True).stdout
    found = set()
    for line in text.splitlines():
        m = re.search(r"\bOBJECT\b.*?::(k_actor_\w+<[^>]*>)\(", line)
        if m:
            found.add(m.group(1).replace(" ", ""))
    return found
