"""numpy restatement of the general CSR operator's kernels (csrc/spmv_kernels.hip), read from their text and not from their outputs:
the launch geometry and the automatic choice, the row sums of the two variants whose order is not the sequential one (csr/adaptive,
csr/wavefront) and the fused p.Ap partials of the stream / adaptive kernels. Test infrastructure: tests/test_csr_restatement.py holds
it against exact sums on the CPU, tests/test_csr_gpu.py compares the kernels with it bit for bit. Everything is float64; a fused
multiply-add is the oracle's fma (numpy's a * b + c rounds twice); the library is built with -ffp-contract=off, so a `+` of the
kernels is a plain add. Row r of the matrix is thread r % per_block of logical block r // per_block.

Also here: the matrices made for these kernels -- adaptive_table(), one scenario of the chunk walk per 16-row block, and arrow(), a
symmetric positive definite matrix with three hub rows for the fused partials and whole solves."""
import collections
import functools

import numpy as np

import cg_restatement as CG
import reduction_restatement as R
from matrices import ENTRY_DTYPE
from oracle import oracle as O

THREADS = 256     # kCsrStreamThreads
PER_THREAD = 4    # kPerThread of csr_stream_kernel<256, 4, ...>
CAP = 1024        # kCsrStreamCap: the LDS strip, one chunk
WAVE = 64
VARIANTS = ("stream", "adaptive", "row-scalar", "wavefront")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ---------------------------------------------------------------- geometry
def stream_geometry(rows, nnz):
    """csr_stream_geometry, its lines `const double avg = rows > 0 ? (double)m.nnz_local / rows : 1.0;`,
    `int per_block = (int)(0.9 * kCsrStreamCap / (avg > 1.0 ? avg : 1.0));`,
    `per_block = per_block > kCsrStreamThreads ? kCsrStreamThreads : (per_block < 16 ? 16 : per_block & ~15);` and
    `*blocks_out = (rows + per_block - 1) / per_block;`: capped at 256, floored at 16, else rounded down to a multiple of 16."""
    avg = float(nnz) / float(rows) if rows > 0 else 1.0
    per_block = int(0.9 * CAP / (avg if avg > 1.0 else 1.0))
    per_block = THREADS if per_block > THREADS else (16 if per_block < 16 else per_block & ~15)
    return per_block, (rows + per_block - 1) // per_block


def auto_variant(rows, nnz, max_row_nnz):
    """csr_auto_variant, its lines `if (mean > 192.0) return CsrVariant::Wavefront;` and
    `return m.max_row_nnz > 1024 ? CsrVariant::Adaptive : CsrVariant::Stream;` with mean = nnz / rows (0.0 without rows)."""
    mean = float(nnz) / float(rows) if rows > 0 else 0.0
    if mean > 192.0:
        return "wavefront"
    return "adaptive" if max_row_nnz > CAP else "stream"


# ---------------------------------------------------------------- row sums
def _fold(v, xg, start):
    """sum = fma(v[k], xg[k], sum) for ascending k, from `start`."""
    s = np.array([start], dtype=np.float64)
    for k in range(len(v)):
        s = O.fma(v[k:k + 1], xg[k:k + 1], s)
    return float(s[0])


def _from_zero(v, xg):
    """The same from +0.0, by the oracle's row loop (oracle_spmv_csr)."""
    if len(v) == 0:
        return 0.0
    return float(O.spmv_csr(np.array([0, len(v)], dtype=np.int32), np.arange(len(v), dtype=np.int32), v, xg)[0])


def _flush_tree(vacc):
    """flush_long_row up to `sum += t`: `w += __shfl_down(w, off)` from 32 down to 1 in each wave, `s_wave[threadIdx.x >> 6] = w`, then
    `double t = s_wave[0]; for (q = 1 ..) t += s_wave[q];`."""
    w = R.wave_tree(vacc.reshape(THREADS // WAVE, WAVE))
    return ((w[0] + w[1]) + w[2]) + w[3]


def adaptive_row_sums(rp, ci, va, x):
    """csr_stream_kernel<256, 4, true> ("csr/adaptive"), alpha = 1. Returns (y, events).

    Per logical block of per_block rows with the span [kb, ke) of entries. A span of at most 1024 entries (the `if` branch of the
    kernel): every row is sum = fma(sv[k], sx[k], sum) from +0.0 in ascending order, O.spmv_csr's sum; event "single:<span>".
    Otherwise (the `else` branch) the span is walked in chunks [base, end) of 1024 from kb:
      - owner = the thread t with k0 <= base and k1 >= end (`if (has_row && k0 <= base && k1 >= end) s_owner[parity] = threadIdx.x;`;
        rows are disjoint, so at most one), else -1; `if (long_owner >= 0 && owner != long_owner) flush_long_row();`
      - a vector run that is open under another owner is flushed first ("F<t>", flush_long_row): t = ((w0 + w1) + w2) + w3 of the four
        wave trees of vacc, sum[owner] = sum[owner] + t, vacc = +0.0 in every thread;
      - owner >= 0, a vector chunk ("V<t>", "V<t>p" when end - base < 1024): vacc[t] = fma(v, x, vacc[t]) for the entries
        base + t + 256 u, u = 0..3; a slot at or past `end` holds v = 0 and x = 0, that is fma(0, 0, vacc[t]);
      - owner < 0, a staged chunk ("S"): every row folds its part [max(k0, base), min(k1, end)) from LDS into its running sum with
        fma in ascending order;
      - a run still open behind the last chunk is flushed.
    A running sum that no flush has reached is a chain of fma from +0.0 over consecutive entries, whatever the chunks were: it is
    evaluated when a flush needs it (the head of a long row) or at the end (every other row), both by the oracle's loop. Behind a
    flush the chain goes on from the flushed value entry by entry (the tail)."""
    rp = np.asarray(rp, dtype=np.int64)
    va, xg = _f64(va), _f64(x)[np.asarray(ci, dtype=np.int64)]
    rows, nnz = len(rp) - 1, int(rp[-1])
    per_block, blocks = stream_geometry(rows, nnz)
    y = O.spmv_csr(rp.astype(np.int32), np.arange(nnz, dtype=np.int32), va, xg) if rows else np.zeros(0)
    lane = np.arange(THREADS, dtype=np.int64)
    events = []
    for g in range(blocks):
        r0, r1 = g * per_block, min((g + 1) * per_block, rows)
        kb, ke = int(rp[r0]), int(rp[r1])
        if ke - kb <= CAP:
            events.append(f"single:{ke - kb}")
            continue
        k0, k1 = rp[r0:r1], rp[r0 + 1:r1 + 1]
        ev = []
        total = {}               # thread -> running sum, once a flush has reached it
        folded_to = {}           # thread -> the entry its running sum has been folded up to
        vacc, long_owner, run_start = np.zeros(THREADS), -1, 0

        def flush():
            nonlocal vacc, long_owner
            t = long_owner
            if t not in total:  # the staged head of the row, folded before the run began
                total[t] = _from_zero(va[k0[t]:run_start], xg[k0[t]:run_start])
            total[t] = float(np.float64(total[t]) + _flush_tree(vacc))
            ev.append(f"F{t}")
            vacc, long_owner = np.zeros(THREADS), -1

        for base in range(kb, ke, CAP):
            end = min(base + CAP, ke)
            covers = np.flatnonzero((k0 <= base) & (k1 >= end))
            assert len(covers) <= 1
            owner = int(covers[0]) if len(covers) else -1
            if long_owner >= 0 and owner != long_owner:
                flush()
            if owner >= 0:
                if long_owner < 0:
                    run_start = base
                for u in range(PER_THREAD):
                    e = base + lane + u * THREADS
                    live = e < end
                    at = np.where(live, e, 0)
                    vacc = O.fma(np.where(live, va[at], 0.0), np.where(live, xg[at], 0.0), vacc)
                long_owner = owner
                folded_to[owner] = end
                ev.append(f"V{owner}" + ("p" if end - base < CAP else ""))
                continue
            ev.append("S")
            for t in total:  # rows behind their flush: the tail
                lo, hi = max(int(k0[t]), base), min(int(k1[t]), end)
                if lo < hi:
                    assert lo == folded_to[t]
                    total[t] = _fold(va[lo:hi], xg[lo:hi], total[t])
                    folded_to[t] = hi
        if long_owner >= 0:
            flush()
        for t, s in total.items():
            assert folded_to[t] == k1[t]
            y[r0 + t] = s
        events.append(" ".join(ev))
    return y, events


def wavefront_row_sums(rp, ci, va, x):
    """csr_wavefront_kernel, alpha = 1: `for (int k = m.row_ptr[row] + lane; k < k1; k += 64) sum = fma(m.values[k], x_at(...), sum);`
    from +0.0 in every lane, then `sum = wave_sum(sum);`, the shuffle tree (R.wave_tree: lane 0's value), stored by lane 0."""
    rp = np.asarray(rp, dtype=np.int64)
    va, xg = _f64(va), _f64(x)[np.asarray(ci, dtype=np.int64)]
    rows = len(rp) - 1
    k0, length = rp[:-1], np.diff(rp)
    lanes = np.zeros((rows, WAVE))
    lane = np.arange(WAVE, dtype=np.int64)
    for step in range(0, int(length.max()) if rows else 0, WAVE):
        on = np.flatnonzero(length > step)  # rows that still have an entry for lane 0
        off = step + lane[None, :]
        live = off < length[on, None]
        at = np.where(live, k0[on, None] + off, 0)
        new = O.fma(va[at], xg[at], lanes[on]).reshape(len(on), WAVE)
        lanes[on] = np.where(live, new, lanes[on])
    return R.wave_tree(lanes)


def row_sums(rp, ci, va, x, variant):
    """A x as the forced variant sums it: stream and row-scalar are the sequential sum (bit for bit, as their kernels' comments say and
    tests/test_spmv_gpu.py holds them), the other two the restatements above."""
    if variant == "adaptive":
        return adaptive_row_sums(rp, ci, va, x)[0]
    if variant == "wavefront":
        return wavefront_row_sums(rp, ci, va, x)
    assert variant in ("stream", "row-scalar"), variant
    return O.spmv_csr(rp, ci, va, x)


def variant_of(rp, name):
    """The restatement's variant word of an operator's variant() ("csr/adaptive"), Auto resolved by auto_variant when name is None."""
    if name is None:
        length = np.diff(rp)
        return auto_variant(len(rp) - 1, int(rp[-1]), int(length.max()) if len(length) else 0)
    return name.split("/", 1)[1]


# ---------------------------------------------------------------- fused partials
def stream_block_partials(x, s, per_block):
    """The dot_partials tail of csr_stream_kernel (`double d = has_row ? x[row] * row_sum : 0.0;`, the shuffle tree, `s_wave`, then
    `t = s_wave[0]; t += s_wave[q]` into `dot_partials[blk]`): logical block g holds rows g * per_block ...; thread t < per_block with a row holds
    the plain product x[row] * s[row] (s = the unscaled row sum), every other of the 256 threads +0.0; the four wave trees, added
    ((w0 + w1) + w2) + w3; slot = logical block."""
    s = _f64(s)
    rows = len(s)
    x = _f64(x)[:rows]
    blocks = (rows + per_block - 1) // per_block
    term = np.zeros((blocks, THREADS))
    r = np.arange(rows)
    term[r // per_block, r % per_block] = x * s
    w = R.wave_tree(term.reshape(blocks, THREADS // WAVE, WAVE))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def system(O_, rp, ci, va, variant):
    """cg_solve_device on cusparse-csr under a forced variant (a cg_restatement.System, device_form): the product is the variant's row
    sums; stream / adaptive write the fused partials above (csr_fused_launch); row-scalar / wavefront have no fused form, so
    slab_spmv (csrc/cg_slab_solve.hip, the loop csrc/cg_single.hip hands an operator to) runs run_device and then launch_dot on
    (p, A p): dot_partials_kernel's streaming partials. r0 comes from cg_init_residual_kernel in every case."""
    assert variant in VARIANTS, variant
    per_block, _ = stream_geometry(len(rp) - 1, int(rp[-1]))
    spmv = lambda v: row_sums(rp, ci, va, v, variant)  # noqa: E731
    if variant in ("stream", "adaptive"):
        return CG.System(spmv, lambda p, ap: (stream_block_partials(p, ap, per_block), ()), CG.stream_rr0, True)
    return CG.System(spmv, lambda p, ap: (R.dot_partials(p, ap), ()), CG.stream_rr0, True)


# ---------------------------------------------------------------- the adaptive table
TABLE_COLS = 6000
RESERVED = 64  # columns [0, 64) and [6000 - 64, 6000): each used at most once, +inf there in the poisoned x
FILL = 3
# (row lengths of one 16-row block, its events, what it exercises)
TABLE_BLOCKS = (
    ([1024] + [FILL] * 15, "V0 F0 S", "a row of exactly one strip, aligned: one vector chunk and nothing else of it"),
    ([64] * 16, "single:1024", "a span of exactly 1024: the last single-chunk case"),
    ([64] * 15 + [65], "S V15p F15", "a span of 1025: a one-entry partial vector chunk in a 65-entry row"),
    ([5, 3500] + [FILL] * 14, "S V1 V1 F1 S", "staged head, two vector chunks, staged tail"),
    ([2048, 2048] + [FILL] * 14, "V0 V0 F0 V1 V1 F1 S", "two long rows meeting at a chunk boundary: the owner changes with no staged chunk between"),
    ([1019, 3000] + [FILL] * 14, "S V1 V1 F1 S", "a long row starting five entries before a chunk boundary"),
    ([FILL] * 15 + [3027], "S V15 V15 F15", "the long row is the block's last and ends on a full chunk: the flush after the loop"),
    ([0, 0, 2500, 0, 2600] + [FILL] * 11, "V2 V2 F2 S V4 F4 S S", "empty rows in front of, between and behind long rows"),
    ([0] * 16, "single:0", "a block of empty rows"),
    ([2100], "V0 V0 V0p F0", "a short last block: one row, partial last vector chunk, dead slots"),
)
TABLE_LONG_ROWS = (0, 47, 49, 64, 65, 81, 111, 114, 116, 144)  # the rows with a V token

Table = collections.namedtuple("Table", "rp ci va x x_poisoned reserved lengths")


def entries_of(rp, ci, va):
    """The CSR as COO entries (what HostMatrix takes), in CSR order."""
    e = np.zeros(len(ci), dtype=ENTRY_DTYPE)
    e["row"], e["col"], e["value"] = np.repeat(np.arange(len(rp) - 1), np.diff(rp)), ci, va
    return e


@functools.lru_cache(maxsize=1)
def adaptive_table():
    """145 rows x 6000 columns, 25 169 entries, every row sorted. The nearest non-empty row in front of each long row ends in a column
    of [5936, 6000), the nearest non-empty row behind it begins with a column of [0, 64); everything else comes from [64, 5936).
    Values uniform in [-3, 3) \\ (-0.25, 0.25), x standard normal; x_poisoned holds +inf at the reserved columns in use: an entry read
    one place in front of or behind a long row's own shows as a non-finite row that holds no such column. The seed is one under which
    columns 0 and 5999 are in use (asserted): a dead slot that gathered x[0], or an index clamped to the last column, meets +inf too.
    Built once, never written."""
    rng = np.random.default_rng(1024)
    lengths = np.array([n for block, _, _ in TABLE_BLOCKS for n in block], dtype=np.int64)
    rows = len(lengths)
    nonempty = np.flatnonzero(lengths > 0)
    first_is_low, last_is_high = set(), set()
    for r in TABLE_LONG_ROWS:
        front, behind = nonempty[nonempty < r], nonempty[nonempty > r]
        if len(front):
            last_is_high.add(int(front[-1]))
        if len(behind):
            first_is_low.add(int(behind[0]))
    low = iter(rng.permutation(RESERVED).tolist())
    high = iter((TABLE_COLS - RESERVED + rng.permutation(RESERVED)).tolist())
    cols, reserved = [], []
    for r in range(rows):
        head = [next(low)] if r in first_is_low else []
        tail = [next(high)] if r in last_is_high else []
        middle = int(lengths[r]) - len(head) - len(tail)
        assert middle >= 0, r
        body = RESERVED + np.sort(rng.choice(TABLE_COLS - 2 * RESERVED, size=middle, replace=False))
        cols.append(np.concatenate([head, body, tail]).astype(np.int32))
        reserved += head + tail
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ci = np.concatenate(cols).astype(np.int32)
    va = rng.uniform(0.25, 3.0, len(ci)) * rng.choice([-1.0, 1.0], len(ci))
    x = rng.standard_normal(TABLE_COLS)
    reserved = np.array(sorted(reserved), dtype=np.int64)
    assert reserved[0] == 0 and reserved[-1] == TABLE_COLS - 1
    xp = x.copy()
    xp[reserved] = np.inf
    for a in (rp, ci, va, x, xp, reserved, lengths):
        a.setflags(write=False)
    return Table(rp, ci, va, x, xp, reserved, lengths)


def hand_made():
    """Two rows whose sums are worked out by hand in integers around 2^53, where one more or one fewer unit shows the order of the
    additions; x is all ones, the values are the products. Returns (rp, ci, va, cols, {variant: {row: value}}).

    16 rows (per_block 16): row 0 holds 1022 zeros, row 1 holds 2 + 1024 + 1 entries, rows 2 .. 15 three ones each. csr/adaptive walks
    "S V1 F1 S": row 1's head [1, 1] is staged with row 0 and gives sum = 2; its next 1024 entries are one vector chunk with 2^53 at
    slot 5, 1 at slots 261 and 517 (lane 5: fma folds 1 into 2^53 twice, 2^53 stays), 1 at slot 64 (wave 1) and at slot 128 (wave 2):
    wave sums 2^53, 1, 1, 0, added in wave order ((2^53 + 1) + 1) + 0 = 2^53; the flush gives 2 + 2^53 = 2^53 + 2; the tail [2] gives
    2^53 + 4. The head folded behind the tree would end at 2^53 + 2, the wave sums added from the last wave down at 2^53 + 6, the two
    ones of lane 5 added to each other first at 2^53 + 6. The sequential sum is 2, 2^53 + 2, then 2^53 + 3 -> 2^53 + 4 (ties to even) at slot
    64, three more ones that leave 2^53 + 4 as it is (2^53 + 5 ties back to it), and 2^53 + 6 behind the tail.

    Row 16 (its own wave under csr/wavefront) holds 65 entries: 2^53 at 0, 1 at 1, 33 and 64. Lane 0 folds entries 0 and 64: 2^53;
    lanes 1 and 33 meet in the tree's first step: 2; the last step adds lanes 0 and 1: 2^53 + 2. The sequential sum is 2^53."""
    big = 2.0 ** 53
    row0 = np.zeros(1022)
    chunk = np.zeros(1024)
    chunk[[5, 261, 517, 64, 128]] = [big, 1.0, 1.0, 1.0, 1.0]
    row1 = np.concatenate([[1.0, 1.0], chunk, [2.0]])
    row16 = np.zeros(65)
    row16[[0, 1, 33, 64]] = [big, 1.0, 1.0, 1.0]
    rows = [row0, row1] + [np.ones(3)] * 14 + [row16]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate([np.arange(len(r)) for r in rows]).astype(np.int32)
    want = {"adaptive": {1: big + 4.0, 16: big}, "stream": {1: big + 6.0, 16: big}, "row-scalar": {1: big + 6.0, 16: big},
            "wavefront": {16: big + 2.0}}
    return rp, ci, np.concatenate(rows), 1100, want


SQUARE_FILL = 60  # 5855 further rows of 60 entries keep the mean above 57.6: per_block stays 16


@functools.lru_cache(maxsize=1)
def table_square():
    """The table made square for the fused partials, which exist on square operators only (fused_spmv_of; the kernel indexes x by the
    row): its 145 rows, then rows 145 .. 5999 of 60 entries each from the unreserved columns. per_block is still 16, so blocks 0 .. 8
    are the table's own scenarios; row 144 now shares block 9 with 15 short rows ("V0 V0 F0 S"). Returns (rp, ci, va)."""
    t = adaptive_table()
    rng = np.random.default_rng(6000)
    more = TABLE_COLS - (len(t.rp) - 1)
    stride = (TABLE_COLS - 2 * RESERVED) // SQUARE_FILL  # one column from each of 60 strata: sorted and distinct
    body = RESERVED + stride * np.arange(SQUARE_FILL)[None, :] + rng.integers(0, stride, (more, SQUARE_FILL))
    rp = np.concatenate([t.rp, t.rp[-1] + SQUARE_FILL * np.arange(1, more + 1)]).astype(np.int32)
    ci = np.concatenate([t.ci, body.ravel()]).astype(np.int32)
    va = np.concatenate([t.va, rng.uniform(0.25, 3.0, body.size) * rng.choice([-1.0, 1.0], body.size)])
    for a in (rp, ci, va):
        a.setflags(write=False)
    return rp, ci, va


# ---------------------------------------------------------------- the arrow matrices
ARROW_SIZES = (3000, 8192)  # per_block 144 and 256 by stream_geometry
ARROW_SPOKES = 2500

Arrow = collections.namedtuple("Arrow", "n rp ci va hubs per_block blocks")


def arrow_hubs(n, per_block):
    """Three hub rows whose thread indices (row % per_block) are 0, one of wave 1, and the last thread of a full block (wave 2 or 3);
    one of them is the matrix's last row."""
    last = n - 1
    hubs = {2 * per_block, 5 * per_block + per_block - 1, last}
    if not any(64 <= h % per_block < 128 for h in hubs):
        hubs.add(3 * per_block + 100)
        hubs.discard(5 * per_block + per_block - 1)  # the last row is then the last thread of its block
    return sorted(hubs)


@functools.lru_cache(maxsize=2)
def arrow(n):
    """Symmetric, diagonal = 1 + the row's absolute off-diagonal sum (positive definite); each hub row is joined to 2500 random rows
    by an edge of one random value in both directions. Sorted CSR, built once, never written."""
    rng = np.random.default_rng(n)
    per_block, _ = stream_geometry(n, n + 6 * ARROW_SPOKES)
    hubs = arrow_hubs(n, per_block)
    edges = {}
    for h in hubs:
        others = np.delete(np.arange(n), h)
        for j, v in zip(rng.choice(others, size=ARROW_SPOKES, replace=False).tolist(), rng.uniform(-1.0, 1.0, ARROW_SPOKES).tolist()):
            edges.setdefault((min(h, j), max(h, j)), v)
    a = np.array([k[0] for k in edges] + [k[1] for k in edges], dtype=np.int64)
    b = np.array([k[1] for k in edges] + [k[0] for k in edges], dtype=np.int64)
    v = np.array(list(edges.values()) * 2)
    diag = 1.0 + np.bincount(a, weights=np.abs(v), minlength=n)
    r = np.concatenate([a, np.arange(n)])
    c = np.concatenate([b, np.arange(n)])
    v = np.concatenate([v, diag])
    order = np.lexsort((c, r))
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    ci, va = c[order].astype(np.int32), v[order]
    per_block, blocks = stream_geometry(n, len(ci))
    for arr in (rp, ci, va):
        arr.setflags(write=False)
    return Arrow(n, rp, ci, va, tuple(hubs), per_block, blocks)
