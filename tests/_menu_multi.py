"""Coverage table of the multi-vector kernel instantiations (a helper: no tests in here), beside tests/_menu.py.

One row per launchable cell (table, dtype, geometry, variant) of the kernels that serve several vectors per pass over A,
with the cases that reach it.  tests/test_kernel_menu_multi.py keeps the set of cells in step with csrc/fos_plan.hip and
csrc/fos_fista.hip and checks on the CPU that every case lands on its cell; tests/test_gpu_kernel_menu_multi.py runs every
case against the fp64 oracle.

table     geometry       variant                        instantiation, chosen by
valu      256x4, 512x4   nvec2..4, nvec2..4-B           gemv_multi_kernel<float, TH, 4, 2, NVEC, 2, BBLOCK>: find_multi - n <= 4096
                                                        / <= 8192, 2..4 handles, run_multi / run_multi_rhs; plain runs on a
                                                        streaming, non-tall, non-wide fp32 plan
p1        RB1, RB2       resid, resid-B, store, store-B residual_batch_mfma_kernel<RB, STORE, BBLOCK> (f32) and
                                                        residual_batch_mfma_bf16_kernel<RB, 128, STORE, BBLOCK> (bf16):
                                                        launch_batch_product - RB 2 from 128 x CUs panel rows; resid:
                                                        residual_batch, residual_batch_rhs, trial_batch; store: the lockstep run
p2        gram           first, acc                     gram_batch_mfma_kernel<float, ACC> / gram_batch_mfma_bf16_kernel<ACC>:
                                                        ACC on the panels after the first (m > 256 x CUs)
cluster   cs4, cs8, cs16 pass                           cluster_pass_kernel<CS>: replan(cluster=True), fp32, strips of 1024 columns
dd        residual       p1                             residual_dd_mfma_kernel<T>: fos_gemv_pair_dd_multi, by storage type
dd        gram           first, acc                     gram_dd_mfma_kernel<T, ACC>: ACC on the panels after the first

The row thresholds scale with the device's CU count, so the cases are built for a CU count: build(cus).  ROWS = build(256)
names the cells (ids, the CPU guard); the GPU tests build the cases for the device they run on.

A case is a tests/_menu.py case (m, n, layout, b, wg; layouts strided, cbview, compact - all borrowed with pad=False) plus
  nv      vectors / handles / columns
  rhs     "b": the problem's b for every column, None: no b, "B": a right-hand side per column (the B block)
  prox    True: the lockstep case is run a second time with alpha1 > 0 against the oracle's prox step
  tune    valu: the streaming geometry the planner picks for n (the workgroup hint needs it named)

Every matrix stays below tests/_menu.py's MAX_BYTES (64 MiB), except the three cluster cells: plan_multi_mfma asks for
(CUs / cs) x CP_ROWS x 8 rows, which at a full last strip (cs x 1024 columns) is 128 MiB on 256 CUs - their cap is
CLUSTER_MAX_BYTES.

Not observable through the C ABI: ||r_j||^2 of a lockstep iteration (every lockstep form closes with finish_part2(f, 0):
status().rr is not written) - product 1's squared norms are checked through the resid cells instead."""
from tests import _menu
from tests._menu import EPC, ESZ, MAX_BYTES, _case, tail_rows

VALU_K = 4                                 # chunks per thread of both multi-vector geometries
VALU_CAP = {256: 4096, 512: 8192}          # find_multi: n <= 4096 -> 256 threads, n <= 8192 -> 512 threads
RB2_ROWS_PER_CU = 128                      # launch_batch_product: the 128-row tile from 128 x CUs panel rows
PANEL_ROWS_PER_CU = 256                    # plan_multi_mfma / ensure_dd_multi: a row panel is at most 256 x CUs rows
TILE_COLS = {"f32": 64, "bf16": 128}       # GB_COLS = BT_COLS, GQ_COLS = BQ_COLS
TILE_ROWS = 64                             # GB_ROWS = DM_ROWS = BT_ROWS
DM_COLS = 64
MFMA_MAX_N = 16384
NV_MAX = 16                                # BT_NV
CP_W, CP_ROWS, CP_MIN_PANELS = 1024, 16, 8
CLUSTER_SIZES = (4, 8, 16)
CLUSTER_MAX_BYTES = 130 << 20
GPU_CUS = 256                              # the CU count ROWS is built for (MI355X)

P1_VARIANTS = ("resid", "resid-B", "store", "store-B")


# ---- the dispatcher's choices, from the constants above (tests/test_kernel_menu_multi.py checks them against the source) ----
def panels(m, cus):
    """Rows of every row panel of plan_multi_mfma / ensure_dd_multi."""
    pr = min(PANEL_ROWS_PER_CU * cus, -(-m // 256) * 256)
    return [min(pr, m - r0) for r0 in range(0, m, pr)]


def split_rows(dtype, m, n, cus, tile_cols=None):
    """Rows per row split of product 2 (gram_rows_per_split / dm_rows_per_split)."""
    pr = min(PANEL_ROWS_PER_CU * cus, -(-m // 256) * 256)
    strips = -(-n // (tile_cols or TILE_COLS[dtype]))
    splits = min(max(1, -(-2 * cus // strips)), max(1, pr // 256))
    return -(-(-(-pr // splits)) // TILE_ROWS) * TILE_ROWS


def rb(rows, cus):
    return 2 if rows >= RB2_ROWS_PER_CU * cus else 1


def is_tall(dtype, n):
    """apply_plan: aligned rows of up to 128 fp32 / 256 bf16 columns plan the chunk-per-lane pass."""
    return n <= _menu.TLR_MAX_N[dtype]


def lockstep_form(dtype, n, nv, rhs):
    """lockstep_route (fos_fista.hip) for plain runs on an aligned, unsharded problem of 65..16384 columns:
    single (one handle: fos_fista_run), valu (find_multi), mfma (run_multi_mfma) or refused (FOS_ERR_UNSUPPORTED)."""
    if nv == 1:
        return "refused" if rhs == "B" else "single"
    if dtype == "f32" and not is_tall(dtype, n) and 2 <= nv <= 4 and n <= VALU_CAP[512]:
        return "valu"
    return "mfma" if nv >= 3 else "refused"


def cluster_size(m, n, cus):
    """plan_multi_mfma with FOS_PLAN_CLUSTER: members per cluster, 0 where the one-read form is not served."""
    need = -(-n // CP_W)
    cs = 0 if need <= 2 else 4 if need <= 4 else 8 if need <= 8 else 16 if need <= 16 else 0
    if cus % 8 or not cs or (cus // 8) % cs or m < (cus // cs) * CP_ROWS * CP_MIN_PANELS:
        return 0
    return cs


def cluster_unreachable(cs, cus):
    """The condition of plan_multi_mfma that shuts cluster size cs out on a device of `cus` CUs (None: reachable)."""
    if cus % 8 or (cus // 8) % cs:
        return f"plan_multi_mfma: p->ncu % 8 == 0 and (p->ncu / 8) % cs == 0 do not hold for {cus} CUs, cs = {cs}"
    return None


def p1_cell(dtype, rows, cus, store, bblock):
    return ("p1", dtype, f"RB{rb(rows, cus)}", ("store" if store else "resid") + ("-B" if bblock else ""))


def valu_cell(n, nv, rhs):
    th = 256 if n <= VALU_CAP[256] else 512
    return ("valu", "f32", f"{th}x{VALU_K}", f"nvec{nv}" + ("-B" if rhs == "B" else ""))


def lockstep_cells(dtype, m, n, nv, cus, rhs, cluster=False):
    """The set of cells one lockstep iteration of nv handles launches."""
    form = lockstep_form(dtype, n, nv, rhs)
    if form == "valu":
        return {valu_cell(n, nv, rhs)}
    if form != "mfma":
        return set()
    if cluster and rhs != "B" and dtype == "f32":
        cs = cluster_size(m, n, cus)
        if cs:
            return {("cluster", "f32", f"cs{cs}", "pass")}
    out = set()
    for i, rows in enumerate(panels(m, cus)):
        out.add(p1_cell(dtype, rows, cus, True, rhs == "B"))
        out.add(("p2", dtype, "gram", "acc" if i else "first"))
    return out


def resid_cells(dtype, m, cus, rhs):
    """residual_batch / residual_batch_rhs / trial_batch: product 1 on all rows at once, nothing stored."""
    return {p1_cell(dtype, m, cus, False, rhs == "B")}


def dd_cells(dtype, m, cus):
    out = {("dd", dtype, "residual", "p1")}
    for i, _ in enumerate(panels(m, cus)):
        out.add(("dd", dtype, "gram", "acc" if i else "first"))
    return out


def case_cells(row, c, cus):
    """The cells case c of `row` launches on a device of `cus` CUs."""
    if row["how"] == "resid":
        return resid_cells(row["dtype"], c["m"], cus, c["rhs"])
    if row["how"] == "dd":
        return dd_cells(row["dtype"], c["m"], cus)
    return lockstep_cells(row["dtype"], c["m"], c["n"], c["nv"], cus, c["rhs"], cluster=row["table"] == "cluster")


# ---- cases --------------------------------------------------------------------------------------------------------------
def _mc(m, n, layout, nv, rhs, **kw):
    return _case(m, n, layout, b=rhs == "b", nv=nv, rhs=rhs, prox=False, **kw)


def _widths(dtype, big):
    """The tile multiple, one chunk short of it, one chunk past the previous multiple: at the widest the matrix-core
    kernels serve and at a narrow one (small row counts), or where 256 x CUs rows still fit MAX_BYTES (big)."""
    t, e = TILE_COLS[dtype], EPC[dtype]
    if big:
        return [3 * t, 3 * t - e, 2 * t + e]
    return [MFMA_MAX_N, MFMA_MAX_N - e, MFMA_MAX_N - t + e, 2 * t, 2 * t - e, t + e]


SMALL_ROWS = (1, 37, 129, 600, 129, 37)      # one row, below a row tile, 1 mod 64, a partial last row split of product 2
LAYOUTS = ("strided", "cbview", "compact")


def _nv_mfma(dtype, n, nv, rhs):
    """nv, or 5 where nv handles would take the VALU pass."""
    return nv if lockstep_form(dtype, n, nv, rhs) == "mfma" else 5


def _small(dtype, rhs_of, lockstep, nvs=(16, 15, 3, 16, 15, 3)):
    out = []
    for j, n in enumerate(_widths(dtype, False)):
        rhs = rhs_of(j)
        nv = _nv_mfma(dtype, n, nvs[j], rhs) if lockstep else nvs[j]
        out.append(_mc(SMALL_ROWS[j], n, LAYOUTS[j % 3], nv, rhs))
    return out


def _rb2(dtype, cus, rhs_of, lockstep, nvs=(16, 15, 3)):
    """One panel of at least 128 x CUs rows: 1 mod 128, a partial last row split, below a row tile past the threshold."""
    base = RB2_ROWS_PER_CU * cus
    out = []
    for j, (n, extra) in enumerate(zip(_widths(dtype, True), (1, 600, 37))):
        rhs = rhs_of(j)
        nv = _nv_mfma(dtype, n, nvs[j], rhs) if lockstep else nvs[j]
        out.append(_mc(base + extra, n, LAYOUTS[j % 3], nv, rhs))
    return out


def _acc(dtype, cus, rhs_of, lockstep=True, nvs=(15, 16)):
    """A second panel of fewer than 64 rows, and one of several row splits (the last one partial)."""
    base = PANEL_ROWS_PER_CU * cus
    w = _widths(dtype, True)
    out = []
    for j, (n, extra) in enumerate(((w[1], 40), (w[2], 600))):
        rhs = rhs_of(j)
        nv = _nv_mfma(dtype, n, nvs[j], rhs) if lockstep else nvs[j]
        out.append(_mc(base + extra, n, LAYOUTS[j % 3], nv, rhs))
    return out


def _valu_cases(th, nvec, bblock):
    """Widths: the capacity, one chunk short of it, one chunk past the previous boundary (132: the narrowest non-tall
    width); a workgroup hint that gives the last workgroup a short share; one row."""
    widths = {256: (4096, 4092, 132), 512: (8192, 8188, 4100)}[th]
    rhs = "B" if bblock else "b"
    out = []
    for j, n in enumerate(widths):
        e = _menu.MENU[_menu.first_fit(_menu.MENU, "f32", n)]
        wg = 7
        out.append(_mc(tail_rows("f32", n, e[3], wg), n, LAYOUTS[j % 3], nvec, rhs, wg=wg, tail=True, tune=e[1:4]))
    n1 = widths[1]
    e = _menu.MENU[_menu.first_fit(_menu.MENU, "f32", n1)]
    out.append(_mc(1, n1, "compact", nvec, "B" if bblock else None, tune=e[1:4]))
    return out


def _cluster_cases(cs, cus):
    """A last strip of one chunk, a full last strip, a member with no column at all (and a last strip of one chunk); the
    fewest rows the planner accepts, a last panel of one row, a partial last panel."""
    rows = (cus // cs) * CP_ROWS * CP_MIN_PANELS
    full = cs * CP_W
    lo = (cs // 2) * CP_W if cs > 4 else 2 * CP_W
    return [_mc(rows + 17, full - CP_W + 4, "strided", 16, "b"), _mc(rows, full, "compact", 5, None),
            _mc(rows + 600, lo + 4, "cbview", 15, "b")]


def _dd_small(dtype):
    e = EPC[dtype]
    w = [MFMA_MAX_N, DM_COLS + e, 3 * DM_COLS, 3 * DM_COLS - e, 2 * DM_COLS + e]
    rows, nvs = (37, 1, 129, 600, 97), (16, 1, 2, 15, 3)
    return [_mc(rows[j], n, LAYOUTS[j % 3], nvs[j], "B") for j, n in enumerate(w)]


def _dd_acc(dtype, cus):
    e = EPC[dtype]
    base = PANEL_ROWS_PER_CU * cus
    return [_mc(base + 40, 3 * DM_COLS - e, "strided", 15, "B"), _mc(base + 600, 2 * DM_COLS + e, "cbview", 16, "B")]


def build(cus):
    rows = []

    def add(table, dtype, geometry, variant, how, cases, unreachable=None):
        rows.append(dict(table=table, dtype=dtype, geometry=geometry, variant=variant, how=how,
                         cases=[] if unreachable else cases, unreachable=unreachable))

    for th in (256, 512):
        for bblock in (False, True):
            for nvec in (2, 3, 4):
                add("valu", "f32", f"{th}x{VALU_K}", f"nvec{nvec}" + ("-B" if bblock else ""), "lockstep",
                    _valu_cases(th, nvec, bblock))
    for dtype in ("f32", "bf16"):
        alt = lambda j: ("b", None)[j % 2]                   # noqa: E731
        blk = lambda j: "B"                                   # noqa: E731
        one = lambda j: "b"                                   # noqa: E731
        resid_nvs = (16, 1, 2, 15, 3, 16)
        add("p1", dtype, "RB1", "resid", "resid", _small(dtype, alt, False, resid_nvs))
        add("p1", dtype, "RB1", "resid-B", "resid", _small(dtype, blk, False, resid_nvs))
        add("p1", dtype, "RB1", "store", "lockstep", _small(dtype, alt, True))
        add("p1", dtype, "RB1", "store-B", "lockstep", _small(dtype, blk, True))
        add("p1", dtype, "RB2", "resid", "resid", _rb2(dtype, cus, alt, False, (16, 1, 3)))
        add("p1", dtype, "RB2", "resid-B", "resid", _rb2(dtype, cus, blk, False, (15, 2, 16)))
        add("p1", dtype, "RB2", "store", "lockstep", _rb2(dtype, cus, one, True))
        add("p1", dtype, "RB2", "store-B", "lockstep", _rb2(dtype, cus, blk, True))
        add("p2", dtype, "gram", "first", "lockstep", _small(dtype, lambda j: ("B", "b")[j % 2], True, (15, 16, 16, 3, 3, 15)))
        add("p2", dtype, "gram", "acc", "lockstep", _acc(dtype, cus, lambda j: ("b", "B")[j % 2]))
    for cs in CLUSTER_SIZES:
        add("cluster", "f32", f"cs{cs}", "pass", "lockstep", _cluster_cases(cs, cus), cluster_unreachable(cs, cus))
    for dtype in ("f32", "bf16"):
        add("dd", dtype, "residual", "p1", "dd", _dd_small(dtype)[:3] + _dd_acc(dtype, cus)[:1])
        add("dd", dtype, "gram", "first", "dd", _dd_small(dtype))
        add("dd", dtype, "gram", "acc", "dd", _dd_acc(dtype, cus))
    # the second run with alpha1 > 0 (the prox step of fista_update_multi_kernel / the per-handle update of the VALU pass): one cell per family
    for key, i in ((("valu", "f32", "256x4", "nvec4"), 1), (("valu", "f32", "512x4", "nvec3-B"), 2),
                   (("p1", "f32", "RB1", "store"), 2), (("p2", "bf16", "gram", "first"), 1),
                   (("cluster", "f32", "cs8", "pass"), 0)):
        for r in rows:
            if (r["table"], r["dtype"], r["geometry"], r["variant"]) == key and r["cases"]:
                r["cases"][i]["prox"] = True
    return rows


ROWS = build(GPU_CUS)
row_id = _menu.row_id


def cells(rows=None):
    return _menu.cells(ROWS if rows is None else rows)


def cap_bytes(row):
    return CLUSTER_MAX_BYTES if row["table"] == "cluster" else MAX_BYTES


def case_bytes(row, c):
    """Bytes of the allocation that holds the case's A (the gap of a strided / column-block layout included)."""
    e = EPC[row["dtype"]]
    lda = c["n"] + (2 * e if c["layout"] in ("strided", "cbview") else 0)
    return c["m"] * lda * ESZ[row["dtype"]]
