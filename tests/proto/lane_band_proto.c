/*
 * lane_band_proto.c — CPU prototype (not shipped) of the OFF-CENTRE 32-row band that genasm_lane_kernel.hip sweeps in
 * its eligible rounds (W = 64, W-O <= 31, every lane's window full: m = n = 64), restated step by step: the band's table
 * (lane_dc_band32), the band form of traceback pass 1 (lane_walk_band32) and the window loop that redoes a window on the
 * full table when the band does not prove it safe (lane_align_codes_band32).  UP, DOWN and SAFE are arguments; the
 * kernel's constants are 10 / 21 / 19.  tests/test_band_proto.py checks it run for run against go_align_codes.
 *
 * Column i (swept 63 .. 0) keeps the rows i - UP .. i + DOWN (UP + DOWN + 1 = 32) as ONE dword, bit 31 <-> row i - UP.
 * The band moves up one row per column, so the recurrence is Hyyro's diagonal form: one shift per column, a 32-bit add.
 * Rows past 63 read Eq = 1, Pv = Mv = 0 (like the bits below a short pattern), rows above 0 read Eq = 0.
 *
 * WHY THE BAND IS NOT CENTRED, AND WHEN A WINDOW IS SAFE.  D[i][j] = the least number of edits that align
 * pattern[j..64) to a prefix of text[i..64).  Write delta = j - i (row - column).  A path that realises D[0][0] starts at
 * delta = 0 and ends in row 64 at a column <= 64: at delta >= 0.  A deletion lowers delta by one, an insertion raises it
 * by one, a diagonal step keeps it.  So
 *     a path that reaches delta = -(UP + 1) has made UP + 1 deletions and still owes UP + 1 insertions: >= 2 UP + 2 edits;
 *     a path that reaches delta = DOWN + 1 has made DOWN + 1 insertions and owes nothing:              >= DOWN + 1 edits.
 * The same holds from any cell (i, j) the traceback stands on: it keeps d == D[i][j], the edits spent so far plus d is
 * D[0][0], and the best completion from there is part of a path of cost D[0][0].  Hence with D[0][0] <= S every cell the
 * walk visits has  -floor(S / 2) <= delta <= S,  and each of the three neighbours it asks about — (i, j+1), (i+1, j),
 * (i+1, j+1): delta + 1, delta - 1, delta — has -floor(S / 2) - 1 <= delta <= S + 1.
 * The band computes, for every cell inside it, the least cost over paths that STAY inside it: an over-estimate of D that is
 * exact wherever an optimal completion stays inside.  Its own D[0][0], d_band, is such an over-estimate, so d_band <= S
 * implies D[0][0] <= S.  For S = SAFE = 19, UP = 10, DOWN = 21:  visited cells have -9 <= delta <= 19, the cells asked about
 * -10 <= delta <= 20, all inside -UP .. DOWN; an optimal completion from a cell asked about that matters (value d - 1) is
 * again part of an optimal path of the window and stays within -9 .. 19: its banded value is exact.  A cell asked about
 * whose true value is not d - 1 has a banded value >= its true value >= d (neighbours differ by at most one and the
 * answer "d - 1" is the minimum), so an over-estimate can only turn a true "== d - 1" into a miss — which the exactness
 * above excludes — and never invents one.  The walk on the band is the walk on the full table.
 * (The centred band 15 / 16 is left by paths of cost >= min(2*15 + 2, 16 + 1) = 17 only; 10 / 21 by cost >= 22.  SAFE = 20 is
 * NOT safe: a visited cell's deletion neighbour can then sit at delta = -11, outside the band, where the dword reads a
 * shifted-in zero; tests/test_band_proto.py::test_ties_on_the_edge_rows has windows that SAFE = 20, or UP = 9, decides wrongly.)
 *
 * d_band = 64 - (the number of columns whose main-diagonal step (i+1, i+1) -> (i, i) is free): bit 32 - UP of Xh | Mv
 * in the coordinates of column i + 1's band.
 *
 * The walk keeps its row RELATIVE to the band's top row: jr = j - (i - UP), starting at UP.  An insertion run adds its
 * length, a diagonal step adds 0, a deletion subtracts 1.  The stop mark (row jlim = W-O: every lane of an eligible round
 * has m = 64) is a per-column constant: bit 31 - (W-O - i + UP), absent where that is below bit 0 — a walk that gets there
 * has made more than DOWN insertions.  Visited cells of a safe window have 1 <= jr <= 29.
 */
#define lane_dc_band32 lane_dc_band32_centred
#define lane_align_codes_band32 lane_align_codes_band32_centred
#define lane_stats_band32 lane_stats_band32_centred
#include "lane_proto.c"
#undef lane_dc_band32
#undef lane_align_codes_band32
#undef lane_stats_band32
#undef BAND32_UP
#undef BAND32_DOWN
#undef BAND32_SAFE

typedef struct lane_stats_band32 { uint64_t windows, banded, escapes, mismatching_safe_windows; uint64_t hist[66]; } lane_stats_band32;

/* -> d_band; V1[i], V0[i] (i < TBL) in BAND coordinates: bit 31 <-> row i - UP (no stop mark) */
static int lane_dc_band32(const uint8_t *t, const uint8_t *q, int TBL, int UP, int DOWN, uint32_t *V1, uint32_t *V0)
{
    uint64_t Tlo = 0, Thi = 0, Plo = 0, Phi = 0;
    for (int k = 0; k < 64; k++) {
        Tlo |= (uint64_t)(t[k] & 1) << k; Thi |= (uint64_t)(t[k] >> 1) << k;
        Plo |= (uint64_t)(q[k] & 1) << k; Phi |= (uint64_t)(q[k] >> 1) << k;
    }
    const uint64_t Rlo = lp_brev64(Plo), Rhi = lp_brev64(Phi);
    /* boundary column 64: rows 64 - UP .. 63 exist (D[64][j] = 64 - j: +1 each), rows 64 .. 64 + DOWN do not */
    uint32_t pv = ~0u << (DOWN + 1), mv = 0;
    int free_diagonals = 0;
    for (int i = 63; i >= 0; i--) {
        const uint64_t sl = 0ull - ((Tlo >> i) & 1), sh = 0ull - ((Thi >> i) & 1);
        const uint64_t Eq64 = ~((Rlo ^ sl) | (Rhi ^ sh));           /* bit 63-k <-> pattern[k] (the kernel reads it from LDS) */
        const int s_old = 63 - (i + 1) - DOWN;                      /* column i + 1's band = full-word bits s_old .. s_old + 31 */
        uint32_t eq;
        if (s_old >= 0) eq = (uint32_t)(Eq64 >> s_old);             /* (rows above 0: zeros come in) */
        else eq = (uint32_t)((Eq64 << (-s_old)) | ((1ull << (-s_old)) - 1ull));     /* rows past 63: Eq = 1 */
        const uint32_t xv = eq | mv;
        const uint32_t d0 = (((eq & pv) + pv) ^ pv) | xv;           /* Xh | Mv: Ph, Mh and the table words come out the same with it */
        const uint32_t ph = mv | ~(d0 | pv);
        const uint32_t mh = pv & d0;
        free_diagonals += (int)((d0 >> (32 - UP)) & 1u);            /* row i of column i + 1's band */
        const uint32_t xvs = xv >> 1;
        const uint32_t pvn = mh | ~(xvs | ph);
        const uint32_t mvn = ph & xvs;
        if (i < TBL) {      /* column i's band sits one bit lower than column i + 1's: Ph, Xh of row j move down with it */
            V1[i] = pvn | (ph >> 1);
            V0[i] = pvn | ~((ph >> 1) | (d0 >> 1));
        }
        pv = pvn; mv = mvn;
    }
    return 64 - free_diagonals;
}

/* band form of the kernel's pass 1 (full windows: jlim = TBL), then lane_tb's tail unchanged */
static int lane_tb_band32(const uint32_t *V1, const uint32_t *V0, int TBL, int UP, size_t *tu, size_t *pu, run_sink *out)
{
    const uint32_t jlim = (uint32_t)TBL;
    uint32_t jr = (uint32_t)UP, ti = 0, nDm = 0, Xm = 0, nIm = 0;
    uint8_t ilen[32];
    for (int i = 0; i < TBL; i++) {
        const int sb = TBL - i + UP;                            /* the stop row in this column's band */
        const uint32_t stop = sb < 32 ? 0x80000000u >> sb : 0u;
        const uint32_t nv1 = ~(V1[i] | stop), v0 = V0[i];
        const uint32_t x = (nv1 | ~v0 | stop) << (jr & 31u);
        const uint32_t ni = lp_ffbh32(x);
        ilen[i] = (uint8_t)ni;
        nIm = lp_alignbit(nIm, x, 31);
        jr += ni;
        const uint32_t nt1 = nv1 << (jr & 31u), t0 = v0 << (jr & 31u);
        nDm = lp_alignbit(nDm, nt1, 31);
        Xm = lp_alignbit(Xm, t0, 31);
        jr += (nt1 >> 31) - 1u;                                 /* diagonal step: 0 (the band moves along), deletion: -1 */
    }
    const uint32_t j = jr + (uint32_t)TBL - (uint32_t)UP;
    const unsigned nsh = 32u - (unsigned)TBL;
    const uint32_t notD = nDm << nsh, Xraw = Xm << nsh, Draw = ~notD, Im = ~nIm << nsh;
    ti = lane_alive_columns(notD, Im, j, jlim, (uint32_t)TBL);
    const uint32_t A = ti ? ~(0xffffffffu >> ti) : 0u;
    const uint32_t D = Draw & A, X = Xraw & A;
    const uint32_t B = ((D ^ (D >> 1)) | (X ^ (X >> 1)) | Im | 0x80000000u) & A;
    const int edits = (int)(j - ti + 2u * (unsigned)__builtin_popcount(D) + (unsigned)__builtin_popcount(X));
    uint32_t E = B | Im;
    while (E) {
        const unsigned c = lp_ffbh32(E);
        const uint32_t bit = 0x80000000u >> c;
        if (Im & bit) sink_push(out, 'I', ilen[c]);
        E &= ~bit;
        unsigned nx = lp_ffbh32(E);
        if (nx > ti) nx = ti;
        if (B & bit) sink_push(out, (D & bit) ? 'D' : ((X & bit) ? 'X' : '='), nx - c);
    }
    *tu = ti; *pu = j;
    return edits;
}

int lane_align_codes_band32(const uint8_t *text, size_t text_len, const uint8_t *read, size_t read_len, int W, int O,
                            int UP, int DOWN, int SAFE,
                            go_run *runs, size_t cap, size_t *n_runs, long long *edit_distance, lane_stats_band32 *ls)
{
    if (W != 64 || O < 33 || O >= W || UP < 1 || DOWN < 1 || UP + DOWN != 31) return GO_ERR_PARAMS;
    run_sink out = { runs, cap, 0, 0 };
    size_t ti = 0, ri = 0; long long total = 0;
    const int TBL = W - O;
    uint64_t V1[64], V0[64];
    uint32_t B1[32], B0[32];
    lane_stats dummy = {0, 0, 0};
    while (ri < read_len) {
        size_t n = text_len - ti < (size_t)W ? text_len - ti : (size_t)W;
        size_t m = read_len - ri < (size_t)W ? read_len - ri : (size_t)W;
        size_t tu, pu;
        int banded = 0;
        ls->windows++;
        if (n == 64 && m == 64) {
            const int d_band = lane_dc_band32(text + ti, read + ri, TBL, UP, DOWN, B1, B0);
            ls->hist[d_band < 0 ? 0 : (d_band > 65 ? 65 : d_band)]++;
            if (d_band <= SAFE) banded = 1; else ls->escapes++;
        }
        lane_dc(text + ti, (int)n, read + ri, (int)m, TBL, V1, V0, &dummy);
        if (banded) {
            /* (the proto also walks the full table and counts the safe windows on which the two walks differ: must stay 0) */
            run_sink o1 = { runs + out.n, cap > out.n ? cap - out.n : 0, 0, 0 };
            size_t tu2, pu2;
            go_run tmp[80]; run_sink o2 = { tmp, 80, 0, 0 };
            const int e2 = lane_tb(V1, V0, (int)m, TBL, &tu2, &pu2, &o2, &dummy);
            const int e1 = lane_tb_band32(B1, B0, TBL, UP, &tu, &pu, &o1);
            int same = e1 == e2 && tu == tu2 && pu == pu2 && o1.n == o2.n;
            for (size_t k = 0; same && k < o1.n && k < o1.cap; k++) same = runs[out.n + k].count == tmp[k].count && runs[out.n + k].op == tmp[k].op;
            if (!same) ls->mismatching_safe_windows++;
            out.n += o1.n; out.overflow |= o1.overflow;
            total += e1;
            ls->banded++;
        } else {
            total += lane_tb(V1, V0, (int)m, TBL, &tu, &pu, &out, &dummy);
        }
        ti += tu; ri += pu;
    }
    *n_runs = out.n; *edit_distance = total;
    return out.overflow ? GO_ERR_CAPACITY : GO_OK;
}

/* What each window of a pair looks like to the kernel's round: trace[k] = d_band of window k if it is full (m = n = 64: the
 * round is eligible as far as this lane goes), -1 if not.  The windows advance as the full table's walk says.  -> the number
 * of windows (those past cap are counted, not written), or a negative GO_ERR_*.  tests/test_gpu_band_table.py replays a
 * wavefront's rounds from these. */
int lane_band_window_trace(const uint8_t *text, size_t text_len, const uint8_t *read, size_t read_len, int W, int O,
                           int UP, int DOWN, int32_t *trace, size_t cap)
{
    if (W != 64 || O < 33 || O >= W || UP < 1 || DOWN < 1 || UP + DOWN != 31) return -1;
    const int TBL = W - O;
    size_t ti = 0, ri = 0, k = 0;
    uint64_t V1[64], V0[64];
    uint32_t B1[32], B0[32];
    lane_stats dummy = {0, 0, 0};
    go_run tmp[160];
    while (ri < read_len) {
        size_t n = text_len - ti < (size_t)W ? text_len - ti : (size_t)W;
        size_t m = read_len - ri < (size_t)W ? read_len - ri : (size_t)W;
        size_t tu, pu;
        const int32_t d = (n == 64 && m == 64) ? lane_dc_band32(text + ti, read + ri, TBL, UP, DOWN, B1, B0) : -1;
        if (k < cap) trace[k] = d;
        k++;
        run_sink o = { tmp, 160, 0, 0 };
        lane_dc(text + ti, (int)n, read + ri, (int)m, TBL, V1, V0, &dummy);
        lane_tb(V1, V0, (int)m, TBL, &tu, &pu, &o, &dummy);
        ti += tu; ri += pu;
    }
    return (int)k;
}
