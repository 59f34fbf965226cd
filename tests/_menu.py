"""Coverage table of the single-pass kernel instantiations (a helper: no tests in here).

One row per launchable cell (table, dtype, geometry, variant) of csrc/fos_plan.hip, with the cases that reach it, or
the planner condition that makes it unreachable.  tests/test_kernel_menu.py keeps the entry lists below in step with
the source (CPU); tests/test_gpu_kernel_menu.py runs every case against the fp64 oracle (GPU).

Variants: with_g, resid, dual (the streaming / tall pass), with_g_il, resid_il, dual_il (interleaved rows), cb (the
column-block pair of a column-sharded problem), dd, dd_il (the fp64-accumulating pass of fos_gemv_pair_dd).

A case is a dict:
  m, n       shape
  layout     compact (contiguous, 16-byte aligned), strided (lda = n + 2 chunks), ragged (lda = n + 1),
             misaligned (contiguous view one element into a flat buffer), cbview (A[:, lo:lo + n] of a wider matrix,
             lo one chunk in); every element outside the operand is NaN
  b          False: b = None
  wg         workgroup hint (tune / tune_dd), 0 = the planner's count
  tail       True: the hint leaves rows_per_wg % R != 0 and a last workgroup that ends in a partial row step
  il         replan(interleave=True) first
  no_tall    replan(no_tall=True) first (narrow widths forced onto a streaming geometry)
"""

EPC = {"f32": 4, "bf16": 8}               # elements per 16-byte chunk
ESZ = {"f32": 4, "bf16": 2}
TLR_MAX_N = {"f32": 128, "bf16": 256}     # chunk-per-lane rows: up to 32 lanes of one chunk
TL_MAX_N = 64                             # row-per-thread / row-per-quad forms
CB_MAX = 16384                            # widest column block
MAX_BYTES = 64 << 20                      # every matrix of the GPU matrix stays below this

# kMenu in source order: (dtype, threads, chunks, rows, macro, DUAL sibling (threads, chunks) of a drained entry)
MENU = [
    ("f32", 64, 1, 4, "ENTRY_D", None), ("f32", 64, 2, 4, "ENTRY_D", None),
    ("f32", 256, 1, 4, "ENTRY_D", None), ("f32", 256, 2, 4, "ENTRY_D", None), ("f32", 256, 3, 2, "ENTRY_D", None),
    ("f32", 256, 4, 2, "ENTRY_D", None), ("f32", 256, 5, 2, "ENTRY_NB_IL", None),
    ("f32", 512, 3, 1, "ENTRY_NB_IL", None), ("f32", 512, 4, 1, "ENTRY_NB_IL", None),
    ("f32", 512, 5, 1, "ENTRY_NB_IL", None), ("f32", 1024, 3, 1, "ENTRY_DRAIN", (512, 6)),
    ("f32", 512, 7, 1, "ENTRY_NB_IL", None), ("f32", 1024, 4, 1, "ENTRY_DRAIN", (512, 8)),
    ("f32", 512, 8, 1, "ENTRY_D", None), ("f32", 1024, 2, 2, "ENTRY", None),
    ("bf16", 64, 1, 4, "ENTRY", None), ("bf16", 64, 2, 4, "ENTRY", None),
    ("bf16", 256, 1, 4, "ENTRY", None), ("bf16", 256, 2, 2, "ENTRY", None),
    ("bf16", 256, 3, 1, "ENTRY_NB_IL", None), ("bf16", 256, 4, 1, "ENTRY_NB_IL", None),
    ("bf16", 256, 5, 1, "ENTRY_IL_ND", None),
    ("bf16", 512, 3, 1, "ENTRY_NB_IL", None), ("bf16", 512, 4, 1, "ENTRY_NB_IL", None),
    ("bf16", 512, 5, 1, "ENTRY_IL_ND", None), ("bf16", 512, 6, 1, "ENTRY_IL_ND", None),
]

# kDdMenu in source order: (dtype, threads, chunks, rows, has the interleaved form)
DD_MENU = [
    ("f32", 64, 1, 4, False), ("f32", 64, 2, 2, False), ("f32", 64, 3, 2, False),
    ("f32", 256, 1, 2, False), ("f32", 256, 2, 2, False), ("f32", 256, 3, 1, False),
    ("f32", 256, 4, 1, True), ("f32", 512, 3, 1, True), ("f32", 512, 4, 1, True), ("f32", 512, 5, 1, True),
    ("f32", 512, 8, 1, True),
    ("bf16", 64, 1, 2, False), ("bf16", 64, 2, 2, False), ("bf16", 256, 1, 2, False), ("bf16", 256, 2, 1, False),
    ("bf16", 256, 3, 1, True), ("bf16", 256, 4, 1, True), ("bf16", 512, 3, 1, True), ("bf16", 512, 4, 1, True),
]

# kTallRows*: lanes per row (a 16-byte chunk per lane)
TALL_ROWS = {"f32": (8, 16, 32), "bf16": (8, 16, 32)}
# kTall*: rows by column capacity (the last row is the row-per-quad kernel), columns by load form
TALL_CAPS = (8, 16, 32, 64)
TALL_FORMS = {"f32": ("DIRECT", "VEC", "STAGE", "STAGE4"), "bf16": ("DIRECT", "STAGE")}

MACRO_VARIANTS = {
    "ENTRY": ("with_g", "resid", "cb"),
    "ENTRY_D": ("with_g", "resid", "dual", "cb"),
    "ENTRY_NB_IL": ("with_g", "resid", "dual", "cb", "with_g_il", "resid_il", "dual_il"),
    "ENTRY_DRAIN": ("with_g", "resid", "dual", "cb", "with_g_il", "resid_il", "dual_il"),
    "ENTRY_IL_ND": ("with_g", "resid", "cb", "with_g_il", "resid_il"),
}
TALL_VARIANTS = ("with_g", "resid", "dual", "dd")


def geo(th, k, r):
    return f"{th}x{k}x{r}"


def cap(dtype, th, k):
    return th * k * EPC[dtype]


def first_fit(entries, dtype, n):
    """Index of the first entry of `dtype` whose capacity is at least n (default_entry / ensure_dd), or None."""
    for i, e in enumerate(entries):
        if e[0] == dtype and cap(dtype, e[1], e[2]) >= n:
            return i
    return None


def prev_cap(entries, dtype, c):
    """Largest capacity of `dtype` below c (0 if none)."""
    return max([cap(dtype, e[1], e[2]) for e in entries if e[0] == dtype and cap(dtype, e[1], e[2]) < c], default=0)


def cb_width(n):
    """fos_problem_set_comm_cols: n rounded up to 64 columns, split into blocks of at most 16384."""
    blocks = (n + CB_MAX - 1) // CB_MAX
    return ((n + blocks - 1) // blocks + 63) // 64 * 64


def min_rows(dtype, n, r, bytes_per_wg=32768):
    """plan_fused (and ensure_dd with 64 KiB): the fewest rows a workgroup is given."""
    row_bytes = n * ESZ[dtype]
    return max(2 * r, -(-bytes_per_wg // row_bytes))


def tail_rows(dtype, n, r, wg, bytes_per_wg=32768):
    """Smallest m >= wg * min_rows for which `wg` workgroups get rows_per_wg % r != 0 and the last one a partial row
    step (r > 1); for r = 1 (no row step to cut) the smallest m giving an uneven last workgroup."""
    m = wg * max(min_rows(dtype, n, r, bytes_per_wg), 4 * r + 1) + 1      # (several row steps per workgroup)
    while True:
        rpw = -(-m // wg)
        last = m - (wg - 1) * rpw
        if -(-m // rpw) == wg and 0 < last < rpw and (r == 1 or (rpw % r and last % r)):
            return m
        m += 1


def _case(m, n, layout, **kw):
    c = dict(m=m, n=n, layout=layout, b=True, wg=0, tail=False, il=False, no_tall=False)
    c.update(kw)
    return c


def _stream_cases(dtype, th, k, r, il):
    """Widths: the capacity, one chunk short of it (the last thread's final chunk is dead), the previous capacity plus
    one chunk (most lanes re-read their chunk 0).  Rows: a tail on an odd workgroup count, and m = 1 without b."""
    c, e = cap(dtype, th, k), EPC[dtype]
    widths = [c, c - e, prev_cap(MENU, dtype, c) + e]
    out = []
    for n in widths:
        wg = 7
        out.append(_case(tail_rows(dtype, n, r, wg), n, "strided", wg=wg, tail=True, il=il,
                         no_tall=n <= TLR_MAX_N[dtype]))
    n1 = c - e
    out.append(_case(1, n1, "compact", b=False, il=il, no_tall=n1 <= TLR_MAX_N[dtype]))
    return out


def _dual_cases(dtype, th, k, r, il):
    c, e = cap(dtype, th, k), EPC[dtype]
    n = c - e
    wg = 7
    return [_case(tail_rows(dtype, n, r, wg), n, "strided", wg=wg, tail=True, il=il, no_tall=n <= TLR_MAX_N[dtype])]


def _cb_cases(i):
    """Widths whose column block lands on kMenu[i]: n = capacity - one chunk (one full-width block), the band's lowest
    width, and for entries above 8192 columns one width with two blocks, the last one short."""
    dtype, th, k, r = MENU[i][:4]
    c, e = cap(dtype, th, k), EPC[dtype]
    lo = max(prev_cap(MENU, dtype, c), TLR_MAX_N[dtype])
    widths = [c - e, lo + e]
    if c > 8192:
        n2 = 2 * (c - 64) - 2 * e            # two blocks of cb_width = c - 64 ... the second 2 chunks short
        widths.append(n2)
    out = []
    for j, n in enumerate(widths):
        m = 150 if n > CB_MAX else 97 + 64 * (j == 1)
        out.append(_case(m, n, "cbview", b=j != 1))
    return out


def _dd_cases(i, il):
    dtype, th, k, r, _ = DD_MENU[i]
    c, e = cap(dtype, th, k), EPC[dtype]
    lo = max(prev_cap(DD_MENU, dtype, c), TLR_MAX_N[dtype])
    out = []
    for n in (c, c - e, lo + e):
        wg = 7
        out.append(_case(tail_rows(dtype, n, r, wg, 65536), n, "strided", wg=wg, tail=True, il=il))
    out.append(_case(1, c - e, "compact", b=False, il=il))
    return out


def _tall_rows_cases(dtype, lpr):
    """Chunk-per-lane rows: aligned rows of lpr/2+1 .. lpr chunks (5..8 for the 8-lane form)."""
    e = EPC[dtype]
    hi = lpr * e
    lo = (lpr // 2 + 1) * e if lpr > 8 else 5 * e
    return [_case(3001, hi, "strided", wg=7), _case(2999, hi - e, "compact", wg=5), _case(1001, lo, "strided", wg=3),
            _case(1, lo, "compact", b=False)]


# load form of kTall* -> (layout, widths in the capacity band)
def _tall_cases(dtype, c, form):
    lo = {8: 1, 16: 9, 32: 17, 64: 33}[c]
    if form == "DIRECT":                        # strided ragged rows
        widths, layout = (c, c - 1, lo), "ragged"
    elif form == "VEC":                         # 16-byte rows at most 4 chunks long
        widths, layout = tuple(n for n in (c, c - 4) if n >= lo), "strided"
    elif form == "STAGE4":                      # contiguous, 16-byte aligned, ragged rows
        widths, layout = (c - 1, c - 3, lo), "compact"
    else:                                       # STAGE: contiguous, misaligned
        widths, layout = (c, c - 1, lo), "misaligned"
    out = [_case(3001 + 2 * j, n, layout, wg=7 - 2 * j) for j, n in enumerate(widths)]
    # one row without b (strided rows need two: a single row is contiguous whatever its stride)
    out.append(_case(1 if layout in ("compact", "misaligned") else 2, widths[-1], layout, b=False))
    return out


TALL_UNREACHABLE = {
    ("f32", 32, "VEC"): "tall_entry: 17..32 columns with n % 4 == 0, lda % 4 == 0 and an aligned A take kTallRowsF32",
    ("f32", 64, "VEC"): "tall_entry: 33..64 columns with n % 4 == 0, lda % 4 == 0 and an aligned A take kTallRowsF32",
    ("f32", 64, "STAGE4"): "tall_entry: the float4 staged copy is chosen only for idx < 3 (at most 32 columns)",
}


def _build():
    rows = []

    def add(table, dtype, geometry, variant, cases=None, unreachable=None, **extra):
        row = dict(table=table, dtype=dtype, geometry=geometry, variant=variant, cases=cases or [],
                   unreachable=unreachable)
        row.update(extra)
        rows.append(row)

    for i, (dtype, th, k, r, macro, sib) in enumerate(MENU):
        g = geo(th, k, r)
        c = cap(dtype, th, k)
        has_dual = "dual" in MACRO_VARIANTS[macro]
        for v in MACRO_VARIANTS[macro]:
            il = v.endswith("_il")
            if v in ("with_g", "resid", "with_g_il", "resid_il"):
                add("kMenu", dtype, g, v, _stream_cases(dtype, th, k, r, il), tune=(th, k, r), has_dual=has_dual)
            elif v in ("dual", "dual_il"):
                add("kMenu", dtype, g, v, _dual_cases(dtype, th, k, r, il), tune=(th, k, r), sibling=sib)
            elif v == "cb":
                first = first_fit(MENU, dtype, c)
                if first != i:
                    add("kMenu", dtype, g, v, unreachable=f"default_entry picks {geo(*MENU[first][1:4])} for every "
                        f"block width up to {c}: same or larger capacity earlier in kMenu")
                elif c > CB_MAX:
                    add("kMenu", dtype, g, v, unreachable=f"cb_width is at most {CB_MAX} columns, below this entry's band")
                else:
                    add("kMenu", dtype, g, v, _cb_cases(i), tune=(th, k, r))
    for i, (dtype, th, k, r, has_il) in enumerate(DD_MENU):
        for v in ("dd", "dd_il") if has_il else ("dd",):
            add("kDdMenu", dtype, geo(th, k, r), v, _dd_cases(i, v == "dd_il"))
    for dtype, lprs in TALL_ROWS.items():
        for lpr in lprs:
            for v in TALL_VARIANTS:
                add(f"kTallRows{'F32' if dtype == 'f32' else 'Bf16'}", dtype, f"lpr{lpr}", v, _tall_rows_cases(dtype, lpr),
                    lanes=lpr)
    for dtype, forms in TALL_FORMS.items():
        for c in TALL_CAPS:
            for form in forms:
                for v in TALL_VARIANTS:
                    why = TALL_UNREACHABLE.get((dtype, c, form))
                    add(f"kTall{'F32' if dtype == 'f32' else 'Bf16'}", dtype, f"{c}/{form}", v,
                        None if why else _tall_cases(dtype, c, form), unreachable=why, lanes=0)
    return rows


ROWS = _build()

# gemv_wide.hpp and the two-pass fallback: one row each per storage type (outside the parsed tables)
EXTRA = [
    dict(table="wide", dtype="f32", geometry="wide", variant="with_g", cases=[_case(96, 20000, "strided"), _case(1, 32768, "compact", b=False)]),
    dict(table="wide", dtype="bf16", geometry="wide", variant="with_g", cases=[_case(90, 24584, "strided"), _case(1, 32768, "compact", b=False)]),
    dict(table="fallback", dtype="f32", geometry="two-pass", variant="with_g", cases=[_case(513, 1023, "ragged"), _case(1, 2050, "misaligned", b=False)]),
    dict(table="fallback", dtype="bf16", geometry="two-pass", variant="with_g", cases=[_case(257, 1021, "ragged"), _case(1, 2050, "misaligned", b=False)]),
]


def cells(rows=None):
    return {(r["table"], r["dtype"], r["geometry"], r["variant"]) for r in (ROWS if rows is None else rows)}


def row_id(r):
    return f"{r['table']}-{r['dtype']}-{r['geometry']}-{r['variant']}"


def reachable():
    return [r for r in ROWS if r["unreachable"] is None]


def dual_fallback():
    """Streaming entries without a DUAL instantiation: fos_fista_grad_dual must take its two-pass route there."""
    out = []
    for dtype, th, k, r, macro, _ in MENU:
        if "dual" not in MACRO_VARIANTS[macro]:
            for il in (False, True) if "with_g_il" in MACRO_VARIANTS[macro] else (False,):
                out.append(dict(table="kMenu", dtype=dtype, geometry=geo(th, k, r), variant="dual_il" if il else "dual",
                                tune=(th, k, r), cases=_dual_cases(dtype, th, k, r, il), unreachable=None))
    return out
