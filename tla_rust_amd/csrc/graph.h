// graph.h — what the state graph (mc_engine_graph) is made of, written once as MC_HD code: the device kernels (engine_graph.h) and the
// host (tests/_graphshim, the graph the kernels must reproduce) run exactly this.
//
//   * seen_find: the read-only lookup of a fingerprint in the seen-set, by seen_insert_t's placement rule (engine_kernels.h).  It
//     yields the POSITION of the slot that holds the key; a side array with one entry per slot maps positions to arena indices.
//   * graph_edge: what one (state, slot) pair contributes to the graph — nothing, a self loop, an edge to a stored state, a successor
//     that is stored nowhere (dropped), or a successor that must be stored and is not (an inconsistency).
//   * graph_state: the slot loop of one expanded state over the two, on the host (the device kernels are this loop with the wavefront's
//     largest nslots as its bound).
// Compiles without HIP (spec_*.h do too).
#pragma once
#include "coverage.h"   // cov_counts: the pairs that count as generated; CovAction<S>: the action of a pair

namespace mc {

// how the kernels are told the table's form (engine_kernels.h: SEEN_SPARSE, MC_SPARSE_SLOTS; engine_graph.h asserts the two agree)
constexpr uint64_t GRAPH_SEEN_SPARSE = 1ull << 63;
#ifndef MC_SPARSE_SLOTS
#define MC_SPARSE_SLOTS 4
#endif
constexpr int GRAPH_PROBE_CAP = 2048;       // seen_insert_t gives up after as many buckets: a key it stored lies within them
constexpr uint64_t GRAPH_ABSENT = ~0ull;

// The search has ended: entries are write-once and a key lives in the first bucket of its probe sequence that had a free slot when it
// arrived — in whichever slot of that bucket (MC_SEEN_ROTATE picks it by the key).  So: the home bucket from the low 32 bits, the whole
// bucket compared; no match and an empty slot = the key was never stored; no match and a full bucket = the next one, wrapping around.
template <int SLOTS>
MC_HD uint64_t seen_find_t(const uint64_t *table, uint64_t nbuckets, uint64_t fp) {
    if (!fp) return GRAPH_ABSENT;   // 0 is the table's EMPTY marker and nobody's key
    uint64_t bk = ((fp & 0xffffffffull) * nbuckets) >> 32;
    for (int probe = 0; probe < GRAPH_PROBE_CAP; ++probe) {
        const uint64_t *line = (const uint64_t *)__builtin_assume_aligned(table + bk * SLOTS, 16);   // (16-byte loads, as the inserts read it)
        uint64_t w[SLOTS];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < SLOTS; ++i) w[i] = line[i];
        int at = -1;
        bool empty = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < SLOTS; ++i) {
            if (w[i] == fp) at = i;
            empty |= w[i] == 0;
        }
        if (at >= 0) return bk * SLOTS + (uint64_t)at;
        if (empty) return GRAPH_ABSENT;
        bk = bk + 1 == nbuckets ? 0 : bk + 1;
    }
    return GRAPH_ABSENT;
}
// seen: the bucket count with the mode bit, as Engine::seen_arg() hands it to every kernel
MC_HD uint64_t seen_find(const uint64_t *table, uint64_t seen, uint64_t fp) {
    if (seen & GRAPH_SEEN_SPARSE) return seen_find_t<MC_SPARSE_SLOTS>(table, seen & ~GRAPH_SEEN_SPARSE, fp);
    return seen_find_t<8>(table, seen, fp);
}

// ---- the edge rule
enum : unsigned {
    GE_NONE = 0,      // the pair generates nothing
    GE_SELF = 1,      // an edge to the expanded state itself
    GE_EDGE = 2,      // an edge to the stored state whose key sits at seen-set position `pos`
    GE_DROPPED = 3,   // a generated successor that is stored nowhere: counted, no edge
    GE_MISSING = 4    // an unflagged, in-model successor that the seen-set does not hold: an inconsistency
};
// st, f: what S::eval returned for the pair; f is the key the expand kernels insert for it (k_expand_insert, k_expand_pairs: the
// fingerprint eval yields, canonical under SYMMETRY already, for every pair that is neither flagged, out of model nor a self loop).
//   * a self loop needs no lookup;
//   * a failed Assert, an evaluation error, a capacity overflow: the pair is generated and HAS no successor state (whatever eval left
//     in f is not a state's key: the hand lowering of pcal_intro leaves the key of the state the step would have reached) — dropped;
//   * out of model (CONSTRAINT) or invariant-breaking: an edge where the state is stored (the lowerings that store invariant-breaking
//     states and check them when they are expanded), dropped otherwise;
//   * everything else was inserted by the search: a miss is GE_MISSING.
MC_HD unsigned graph_edge(unsigned st, uint64_t f, const uint64_t *table, uint64_t seen, uint64_t &pos) {
    pos = GRAPH_ABSENT;
    if (!cov_counts(st)) return GE_NONE;
    if (st & (ST_ASSERT | ST_SPECERR | ST_OVERFLOW)) return GE_DROPPED;
    if (st & ST_SELFLOOP) return GE_SELF;
    pos = seen_find(table, seen, f);
    if (pos != GRAPH_ABSENT) return GE_EDGE;
    return (st & (ST_OUT_OF_MODEL | ST_INVARIANT)) ? GE_DROPPED : GE_MISSING;
}

// One expanded state on the host: on(kind, position, action id, slot) once per pair that counts, in slot order.
template <class S, class On>
inline void graph_state(const typename S::Params &prm, CWordRef s, const uint64_t *table, uint64_t seen, On &&on) {
    typename S::Local loc;
    S::load(prm, s, loc);
    const int ns = S::nslots(prm, loc);
    for (int slot = 0; slot < ns; ++slot) {
        uint64_t f = 0, pos;
        const unsigned st = S::eval(prm, loc, s, slot, f);
        const unsigned kind = graph_edge(st, f, table, seen, pos);
        if (kind != GE_NONE) on(kind, pos, CovAction<S>::of(prm, loc, s, slot), slot);
    }
}

}  // namespace mc
