/*
 * lane_band_rebase_proto.c — CPU prototype (not shipped) of the band table's kept columns held in the coordinates of the
 * column to their RIGHT.  Everything else is lane_band_proto.c's (included below: the sweep's recurrence, the proof of the
 * band, the full table, the window loop); tests/test_band_rebase_proto.py replays that file's data sets through this one.
 *
 * lane_dc_band32 keeps, for column i < W-O,  V1 = Pv' | Ph  and  V0 = Pv' | ~(Ph | D0)  with bit 31 <-> row i - UP.  Pv'
 * comes out of the sweep in column i's coordinates, Ph and D0 in column i + 1's, one bit higher, so both are shifted down:
 * two shifts per kept column.  Here the words stay in column i + 1's coordinates, bit 31 <-> row i + 1 - UP:
 *     V1 = (Pv' + Pv') | Ph        V0 = (Pv' + Pv') | ~(Ph | D0)
 * one addition.  Against the words of lane_dc_band32 these have lost the band's top row, delta = row - column = -UP, and
 * gained a bit 0, delta = DOWN + 1, that means nothing: Pv' has no such row (a zero comes in), Ph and D0 carry column i + 1's
 * row i + 1 + DOWN there.
 *
 * WHY NEITHER IS READ.  The walk reads a column's words at the rows of the cells it VISITS and nowhere else: the
 * insertion run is the count of leading zeros from the visited row downwards — every row it passes is a visited cell, and
 * so is the row whose set bit ends the count — and the step out of the column is the sign of both words at the visited
 * row.  (The NEIGHBOURS it asks about, one row or one column further, are what those bits encode; their own table bits are
 * not touched.)  By lane_band_proto.c's argument the visited cells of a window with d_band <= SAFE = 19 have
 * -9 <= delta <= 19, inside -UP + 1 .. DOWN for UP = 10, DOWN = 21.  The recurrence itself is untouched — the sweep still
 * carries the row at delta = -UP, which the cells at -UP + 1 need for their deletion neighbour — only the kept copy drops it.
 *
 * The walk's relative row is now j - (i + 1 - UP): it starts at UP - 1, the stop marks sit one bit higher, and after W-O
 * columns the row is j - (W-O - UP + 1).  Visited cells of a safe window have 0 <= jr <= 28.
 *
 * `low` says what the meaningless bit 0 holds, so that the test can show that nothing depends on it: 0 as computed,
 * 1 .. 4 forced to (V1, V0) = (0, 0), (0, 1), (1, 0), (1, 1).
 */
#include "lane_band_proto.c"

/* -> d_band; V1[i], V0[i] (i < TBL) in the coordinates of column i + 1's band: bit 31 <-> row i + 1 - UP (no stop mark) */
static int lane_dc_band32_rebased(const uint8_t *t, const uint8_t *q, int TBL, int UP, int DOWN, int low, uint32_t *V1, uint32_t *V0)
{
    uint64_t Tlo = 0, Thi = 0, Plo = 0, Phi = 0;
    for (int k = 0; k < 64; k++) {
        Tlo |= (uint64_t)(t[k] & 1) << k; Thi |= (uint64_t)(t[k] >> 1) << k;
        Plo |= (uint64_t)(q[k] & 1) << k; Phi |= (uint64_t)(q[k] >> 1) << k;
    }
    const uint64_t Rlo = lp_brev64(Plo), Rhi = lp_brev64(Phi);
    uint32_t pv = ~0u << (DOWN + 1), mv = 0;
    int free_diagonals = 0;
    for (int i = 63; i >= 0; i--) {
        const uint64_t sl = 0ull - ((Tlo >> i) & 1), sh = 0ull - ((Thi >> i) & 1);
        const uint64_t Eq64 = ~((Rlo ^ sl) | (Rhi ^ sh));
        const int s_old = 63 - (i + 1) - DOWN;
        uint32_t eq;
        if (s_old >= 0) eq = (uint32_t)(Eq64 >> s_old);
        else eq = (uint32_t)((Eq64 << (-s_old)) | ((1ull << (-s_old)) - 1ull));
        const uint32_t xv = eq | mv;
        const uint32_t d0 = (((eq & pv) + pv) ^ pv) | xv;
        const uint32_t ph = mv | ~(d0 | pv);
        const uint32_t mh = pv & d0;
        free_diagonals += (int)((d0 >> (32 - UP)) & 1u);
        const uint32_t xvs = xv >> 1;
        const uint32_t pvn = mh | ~(xvs | ph);
        const uint32_t mvn = ph & xvs;
        if (i < TBL) {      /* kept where Ph and D0 are: Pv' moves up a bit instead */
            const uint32_t pv2 = pvn + pvn;
            V1[i] = pv2 | ph;
            V0[i] = pv2 | ~(ph | d0);
            if (low) {
                V1[i] = (V1[i] & ~1u) | (uint32_t)((low - 1) >> 1);
                V0[i] = (V0[i] & ~1u) | (uint32_t)((low - 1) & 1);
            }
        }
        pv = pvn; mv = mvn;
    }
    return 64 - free_diagonals;
}

/* lane_tb_band32 with the row relative to column i + 1's band */
static int lane_tb_band32_rebased(const uint32_t *V1, const uint32_t *V0, int TBL, int UP, size_t *tu, size_t *pu, run_sink *out)
{
    const uint32_t jlim = (uint32_t)TBL;
    uint32_t jr = (uint32_t)UP - 1u, ti = 0, nDm = 0, Xm = 0, nIm = 0;
    uint8_t ilen[32];
    for (int i = 0; i < TBL; i++) {
        const int sb = TBL - i + UP - 1;                        /* the stop row in these coordinates */
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
        jr += (nt1 >> 31) - 1u;
    }
    const uint32_t j = jr + (uint32_t)TBL - ((uint32_t)UP - 1u);
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

/* lane_align_codes_band32 on the re-based words: a safe window is walked on them AND on the full table, and a window on which
 * the two differ in anything — edits, advance, a run — is counted (must stay 0) */
int lane_align_codes_band32_rebased(const uint8_t *text, size_t text_len, const uint8_t *read, size_t read_len, int W, int O,
                                    int UP, int DOWN, int SAFE, int low,
                                    go_run *runs, size_t cap, size_t *n_runs, long long *edit_distance, lane_stats_band32 *ls)
{
    if (W != 64 || O < 33 || O >= W || UP < 2 || DOWN < 1 || UP + DOWN != 31 || low < 0 || low > 4) return GO_ERR_PARAMS;
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
            const int d_band = lane_dc_band32_rebased(text + ti, read + ri, TBL, UP, DOWN, low, B1, B0);
            ls->hist[d_band < 0 ? 0 : (d_band > 65 ? 65 : d_band)]++;
            if (d_band <= SAFE) banded = 1; else ls->escapes++;
        }
        lane_dc(text + ti, (int)n, read + ri, (int)m, TBL, V1, V0, &dummy);
        if (banded) {
            run_sink o1 = { runs + out.n, cap > out.n ? cap - out.n : 0, 0, 0 };
            size_t tu2, pu2;
            go_run tmp[80]; run_sink o2 = { tmp, 80, 0, 0 };
            const int e2 = lane_tb(V1, V0, (int)m, TBL, &tu2, &pu2, &o2, &dummy);
            const int e1 = lane_tb_band32_rebased(B1, B0, TBL, UP, &tu, &pu, &o1);
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
