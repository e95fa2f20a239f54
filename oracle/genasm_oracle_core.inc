/*
 * genasm_oracle_core.inc — TEST INFRASTRUCTURE ONLY.  The windowed GenASM restatement of
 * genasm_oracle.c, written once and instantiated per bitvector type:
 *   GO_BV       type holding one bitvector (uint64_t, unsigned __int128, or the 4-word struct go_bv256)
 *   GO_BV_BITS  its width, GO_BV_MAXW the largest window it serves, GO_NAME(x) the name suffix,
 *   GO_ONES() GO_ZERO() GO_SHL(v,s) GO_OR(a,b) GO_AND(a,b) GO_CLRBIT(v,b) GO_BIT0(v,b)  its operations
 *               (s, b < GO_BV_BITS).
 * The reference keeps W-bit vectors in arrays of 32-bit elements (src/bitvector.hpp:45-48, 124-139);
 * bits at or above m never influence the bits the algorithm inspects (left shifts only), so a wider
 * integer gives identical results.
 */

typedef struct GO_NAME(go_scratch_s) {
    GO_BV R[GO_BV_MAXW + 1][GO_BV_MAXW + 1]; /* R[d][i] */
} GO_NAME(go_scratch);

static inline GO_BV GO_NAME(shl64)(GO_BV v, unsigned s)
{
    /* bitvector::operator<< yields zero once the shift reaches the width
     * (src/bitvector.hpp:116-122). */
    return s >= GO_BV_BITS ? GO_ZERO() : GO_SHL(v, s);
}

static inline int GO_NAME(bit_is_zero)(GO_BV v, unsigned b)
{
    return GO_BIT0(v, b); /* has_zero_at, src/bitvector.hpp:163-175 */
}

/* Pattern masks, genasm_cpu.cpp:178-198. */
static void GO_NAME(pattern_masks)(const uint8_t *pattern, size_t m, GO_BV pm[4])
{
    pm[0] = pm[1] = pm[2] = pm[3] = GO_ONES();
    for (size_t b = 0; b < m; b++)
        pm[pattern[m - 1 - b]] = GO_CLRBIT(pm[pattern[m - 1 - b]], (unsigned)b);
}

/*
 * Distance calculation, genasm_cpu.cpp:210-288: rows d = 0..K, columns
 * i = n..0, stops at the first row whose column 0 has bit m-1 clear
 * (EARLY_TERMINATION, :278-283).  Returns that row, or -1 if none exists
 * (cannot happen while K >= m, since m insertions always work).
 */
static int GO_NAME(distance_sweep)(const uint8_t *text, size_t n,
                          const uint8_t *pattern, size_t m, int K,
                          GO_NAME(go_scratch) *s, go_stats *st)
{
    GO_BV pm[4];
    GO_NAME(pattern_masks)(pattern, m, pm);

    for (int d = 0; d <= K; d++) {
        GO_BV *row = s->R[d];
        const GO_BV *up = d ? s->R[d - 1] : NULL;

        /* column n: nothing of the text left, only insertions (:239-245) */
        row[n] = d ? GO_NAME(shl64)(GO_ONES(), (unsigned)d) : GO_ONES();

        for (size_t i = n; i-- > 0;) {
            GO_BV match = GO_OR(GO_SHL(row[i + 1], 1u), pm[text[i]]);
            if (d == 0) {
                row[i] = match; /* :232-238 */
            } else {
                GO_BV sub = GO_SHL(up[i + 1], 1u);
                GO_BV ins = GO_SHL(up[i], 1u);
                GO_BV del = up[i + 1];
                row[i] = GO_AND(GO_AND(match, sub), GO_AND(ins, del)); /* :246-252 */
            }
        }
        if (st)
            st->dc_cells += n + 1;
        if (GO_NAME(bit_is_zero)(row[0], (unsigned)(m - 1)))
            return d;
    }
    return -1;
}

/*
 * Traceback of one window, genasm_cpu.cpp:290-409.  Walks from (i,j,d) =
 * (0,0,window distance); stops when the pattern is used up or either index
 * reaches W-O (:307-310).  Edit preference: insertion, deletion,
 * substitution, match (:346-370); the last pattern character has its own
 * rule (:336-343).  Runs are flushed per window and never merged with the
 * next window's (:304-305, 400-403).
 */
static int GO_NAME(traceback)(const GO_NAME(go_scratch) *s, size_t n, size_t m, int dist,
                     size_t limit, size_t *text_used, size_t *pattern_used,
                     run_sink *out, go_stats *st)
{
    size_t i = 0, j = 0;
    int d = dist;
    char cur = 0;
    unsigned cur_len = 0;

    while (j < m && i < limit && j < limit) {
        int room = d > 0;
        int text_left = i < n;
        int ins, del, sub;

        if (j + 1 < m) {
            unsigned bj = (unsigned)(m - 1 - j);      /* TB_BIT(j), :59 */
            unsigned bj1 = bj - 1;                    /* TB_BIT(j+1) */
            ins = room && GO_NAME(bit_is_zero)(s->R[d - 1][i], bj1);
            del = room && text_left && GO_NAME(bit_is_zero)(s->R[d - 1][i + 1], bj);
            sub = room && text_left && GO_NAME(bit_is_zero)(s->R[d - 1][i + 1], bj1);
        } else {
            ins = room;
            del = 0;
            sub = room && text_left;
        }

        char op;
        if (ins)      { op = 'I'; j++; d--; }
        else if (del) { op = 'D'; i++; d--; }
        else if (sub) { op = 'X'; i++; j++; d--; }
        else          { op = '='; i++; j++; }

        if (op == cur) {
            cur_len++;
        } else {
            if (cur_len)
                sink_push(out, cur, cur_len);
            cur = op;
            cur_len = 1;
        }
        if (st)
            st->tb_steps++;
    }
    if (cur_len)
        sink_push(out, cur, cur_len);

    *text_used = i;
    *pattern_used = j;
    return dist - d;
}

static int GO_NAME(go_align_codes)(const uint8_t *text, size_t text_len,
                   const uint8_t *read, size_t read_len,
                   int W, int O,
                   go_run *runs, size_t cap, size_t *n_runs,
                   long long *edit_distance, go_stats *stats)
{
    /* W - O > 255 (256/0 alone): a window that is one run would need a count of 256 in the run's count byte; the
     * reference's own uint8_t counter wraps there (genasm_cpu.cpp:305, 388-401) and drops the run, so it is refused */
    if (W < 2 || W > GO_BV_MAXW || O < 0 || O >= W || W - O > 255)
        return GO_ERR_PARAMS;

    /* per-thread table, like the per-thread R of genasm_cpu.cpp:444 */
    static _Thread_local GO_NAME(go_scratch) scratch;
    GO_NAME(go_scratch) *s = &scratch;

    run_sink out = { runs, cap, 0, 0 };
    size_t ti = 0, ri = 0;
    long long total = 0;
    const size_t limit = (size_t)(W - O);

    /* window loop, genasm_cpu.cpp:411-438 */
    while (ri < read_len) {
        size_t n = text_len - ti < (size_t)W ? text_len - ti : (size_t)W;
        size_t m = read_len - ri < (size_t)W ? read_len - ri : (size_t)W;

        int dist = GO_NAME(distance_sweep)(text + ti, n, read + ri, m, W, s, stats);
        if (dist < 0) /* unreachable with K == W */
            return GO_ERR_PARAMS;
        if (stats)
            stats->windows++;

        size_t tu, pu;
        total += GO_NAME(traceback)(s, n, m, dist, limit, &tu, &pu, &out, stats);
        ti += tu;
        ri += pu;
    }

    if (n_runs)
        *n_runs = out.n;
    if (edit_distance)
        *edit_distance = total;
    if (stats) {
        stats->runs += out.n;
        stats->text_used += ti;
    }
    return out.overflow ? GO_ERR_CAPACITY : GO_OK;
}
