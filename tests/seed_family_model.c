/* TEST INFRASTRUCTURE ONLY -- seed families on the oracle's MemHash.
 *
 * progressiveMauve's pairwiseAnchorSearch (ProgressiveAligner.cpp:619-653) runs, on one
 * MemHash, Clear() and then per seed rank ClearSequences() + FindMatches().  ClearSequences
 * (MemHash.cpp:71-74) is MatchFinder::Clear only: mem_table, mem_table_count, m_mem_count and
 * m_collision_count survive, so every round's AddHashEntry calls meet the earlier rounds'
 * entries.  This file includes the oracle unchanged and loops its find_match_seeds over the
 * rounds on ONE memhash_t: buckets, pool, spool and the counters are kept, the SortedMerLists,
 * keys and the extension context are rebuilt per round (as in oracle_find_matches).
 *
 * PairwiseMatchFinder rounds: the reference sorts a seed group by sequence id before it hashes
 * the pairs (match_list.sort(&idmer_id_lessthan), PairwiseMatchFinder.cpp:39).  The table does
 * not depend on the order of one group's calls (their pairs differ in the sequences present),
 * the match log does.  The oracle's enumerate_pairwise once kept the merge's run order, so such
 * a round first records the oracle's AddHashEntry calls (its record mode), puts every group's
 * calls in the reference's order -- by (first, second) sequence of the pair; a group's calls are
 * consecutive and linked by a shared (sequence, position), which no two groups share -- and then
 * makes the calls.  The oracle sorts by sequence id itself now (tests/test_gpu_rearranged.py found
 * its match log out of order on rearranged genomes); the reordering here is kept as a second,
 * independent statement of the order and changes nothing.
 */
#include "../oracle/mums_oracle.c"

/* the sequences of a pair row, as one sort key */
static int pair_key(const int64_t* row, int G) {
    int a = -1, b = -1;
    for (int g = 0; g < G; ++g)
        if (row[g] != 0) { if (a < 0) a = g; else b = g; }
    return a * 64 + b;
}

static int rows_linked(const int64_t* x, const int64_t* y, int G) {
    for (int g = 0; g < G; ++g)
        if (x[g] != 0 && (x[g] == y[g] || x[g] == -y[g])) return 1;
    return 0;
}

/* rows [0, n) of W = G + 1 int64 in the oracle's call order -> the reference's: every seed
 * group's rows (a maximal run in which each row is linked to an earlier one of the run)
 * insertion-sorted by pair_key */
static void pairwise_reference_order(int64_t* rows, uint64_t n, int G) {
    const uint64_t W = (uint64_t)G + 1;
    int64_t* tmp = (int64_t*)malloc(W * sizeof(int64_t));
    uint64_t a = 0;
    while (a < n) {
        uint64_t b = a + 1;
        for (; b < n; ++b) {
            int linked = 0;
            for (uint64_t k = a; k < b && !linked; ++k) linked = rows_linked(rows + k * W, rows + b * W, G);
            if (!linked) break;
        }
        for (uint64_t i = a + 1; i < b; ++i) {
            memcpy(tmp, rows + i * W, W * sizeof(int64_t));
            uint64_t j = i;
            while (j > a && pair_key(rows + (j - 1) * W, G) > pair_key(tmp, G)) {
                memcpy(rows + j * W, rows + (j - 1) * W, W * sizeof(int64_t));
                --j;
            }
            memcpy(rows + j * W, tmp, W * sizeof(int64_t));
        }
        a = b;
    }
    free(tmp);
}

typedef struct {
    uint64_t count;          /* entries of the table after the round (GetMatchList)      */
    uint64_t mem_count;      /* m_mem_count, cumulative                                   */
    uint64_t collisions;     /* m_collision_count, cumulative                             */
    uint64_t probes;         /* AddHashEntry calls of this round                          */
    uint64_t log_n;          /* inserts of this round, in call order (SetMatchLog)        */
    uint64_t* lengths;       /* [count], bucket-major                                     */
    int64_t* starts;         /* [count * G]                                               */
    uint32_t* table_counts;  /* [table_size], mem_table_count                             */
    uint64_t* log_len;       /* [log_n]                                                   */
    int64_t* log_s;          /* [log_n * G]                                               */
} sf_round;

/* rounds r = 0 .. nrounds-1 on sequences seqs[r * G + g] (lens likewise) with prms[r]; every
 * round must use table_size.  Returns 0, or -1 when a round's input is rejected. */
int seed_family_run(int G, uint32_t table_size, int nrounds, const char* const* seqs, const uint64_t* lens,
                    const oracle_params* prms, sf_round* out) {
    if (G < 1 || G > 64 || table_size == 0) return -1;
    memhash_t h;
    memset(&h, 0, sizeof(h));
    h.table_size = table_size;
    h.buckets = (bucket_t*)calloc(table_size, sizeof(bucket_t));
    h.scratch = (int64_t*)malloc((size_t)G * sizeof(int64_t));
    int bad = 0;
    memset(out, 0, (size_t)nrounds * sizeof(sf_round));
    for (int r = 0; r < nrounds && !bad; ++r) {
        const oracle_params* prm = &prms[r];
        const char* const* sq = seqs + (size_t)r * (size_t)G;
        const uint64_t* ln = lens + (size_t)r * (size_t)G;
        oracle_result* res = (oracle_result*)calloc(1, sizeof(oracle_result));
        res->G = G;
        sml_ctx* ctx = (sml_ctx*)calloc((size_t)G, sizeof(sml_ctx));
        uint32_t** words = (uint32_t**)calloc((size_t)G, sizeof(uint32_t*));
        uint64_t** keys = (uint64_t**)calloc((size_t)G, sizeof(uint64_t*));
        bmer_t** sml = (bmer_t**)calloc((size_t)G, sizeof(bmer_t*));
        uint64_t* m = (uint64_t*)calloc((size_t)G, sizeof(uint64_t));
        uint64_t* gbase = (uint64_t*)calloc((size_t)G + 1, sizeof(uint64_t));
        for (int g = 0; g < G && !bad; ++g) {
            if (sml_init(&ctx[g], sq[g], ln[g], prm->seed, &words[g])) { bad = 1; break; }
            m[g] = sml_length(ln[g], ctx[g].L);
            keys[g] = (uint64_t*)malloc((m[g] ? m[g] : 1) * sizeof(uint64_t));
            for (uint64_t p = 0; p < m[g]; ++p) keys[g][p] = get_dna_seed_mer(&ctx[g], p);
            sml[g] = build_sml(&ctx[g], keys[g], m[g]);
            gbase[g + 1] = gbase[g] + m[g];
        }
        if (!bad) {
            h.x.G = G;
            h.x.L = ctx[0].L;
            h.x.seed_mask = ctx[0].seed_mask;
            h.x.keys = (const uint64_t**)keys;
            h.x.n = ln;
            h.x.gnseqi_end = prm->gnseqi_end_neg1 ? (int64_t)-1 : INT64_MAX;
            h.gbase = gbase;
            const uint64_t pool0 = h.pool_n, probes0 = h.probes;
            if (prm->pairwise) {   /* record the calls, order them as the reference, make them */
                h.rec_cap = 1024;
                h.rec_n = 0;
                h.rec = (int64_t*)malloc(h.rec_cap * ((size_t)G + 1) * sizeof(int64_t));
                find_match_seeds(&h, prm, G, sml, m, ln, prm->start_points, res);
                h.rec_cap = 0;
                h.probes = probes0;
                pairwise_reference_order(h.rec, h.rec_n, G);
                for (uint64_t k = 0; k < h.rec_n; ++k) {
                    mhe_t p;
                    memcpy(h.scratch, h.rec + k * ((uint64_t)G + 1), (size_t)G * sizeof(int64_t));
                    p.s = h.scratch;
                    p.len = h.x.L;
                    p.mersize = h.x.L;
                    p.offset = h.rec[k * ((uint64_t)G + 1) + (uint64_t)G];
                    add_hash_entry(&h, &p);
                }
                free(h.rec);
                h.rec = NULL;
                h.rec_n = 0;
            } else {
                find_match_seeds(&h, prm, G, sml, m, ln, prm->start_points, res);
            }
            sf_round* o = &out[r];
            o->count = h.mem_count;
            o->mem_count = h.mem_count;
            o->collisions = h.collisions;
            o->probes = h.probes - probes0;
            o->lengths = (uint64_t*)malloc((o->count ? o->count : 1) * sizeof(uint64_t));
            o->starts = (int64_t*)malloc((o->count ? o->count : 1) * (size_t)G * sizeof(int64_t));
            o->table_counts = (uint32_t*)malloc((size_t)table_size * sizeof(uint32_t));
            uint64_t k = 0;
            for (uint32_t b = 0; b < table_size; ++b) {   /* GetMatchList: MemHash.h:182-203 */
                o->table_counts[b] = h.buckets[b].n;
                for (uint32_t i = 0; i < h.buckets[b].n; ++i, ++k) {
                    const mhe_t* e = &h.pool[h.buckets[b].v[i]];
                    o->lengths[k] = (uint64_t)e->len;
                    memcpy(o->starts + k * (uint64_t)G, e->s, (size_t)G * sizeof(int64_t));
                }
            }
            /* every AddHashEntry insert appends one pool entry: pool order = call order */
            o->log_n = h.pool_n - pool0;
            o->log_len = (uint64_t*)malloc((o->log_n ? o->log_n : 1) * sizeof(uint64_t));
            o->log_s = (int64_t*)malloc((o->log_n ? o->log_n : 1) * (size_t)G * sizeof(int64_t));
            for (uint64_t i = 0; i < o->log_n; ++i) {
                o->log_len[i] = (uint64_t)h.pool[pool0 + i].len;
                memcpy(o->log_s + i * (uint64_t)G, h.pool[pool0 + i].s, (size_t)G * sizeof(int64_t));
            }
        }
        for (int g = 0; g < G; ++g) { free(words[g]); free(keys[g]); free(sml[g]); }
        free(ctx); free(words); free(keys); free(sml); free(m); free(gbase);
        oracle_result_free(res);
    }
    for (uint32_t b = 0; b < table_size; ++b) free(h.buckets[b].v);
    free(h.buckets); free(h.pool); free(h.spool); free(h.scratch); free(h.cm); free(h.hl);
    free(h.plog_bucket); free(h.plog_ref);
    return bad ? -1 : 0;
}

void seed_family_free(sf_round* out, int nrounds) {
    for (int r = 0; r < nrounds; ++r) {
        free(out[r].lengths); free(out[r].starts); free(out[r].table_counts);
        free(out[r].log_len); free(out[r].log_s);
    }
}
