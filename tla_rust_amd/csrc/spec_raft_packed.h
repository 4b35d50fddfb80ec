// spec_raft_packed.h — the raft lowering of spec_raft.h with its rows stored in fewer words (one-GPU engines).
//
// SpecRaft<NS> keeps voterLog[i] in a word of its own per server (NS * lb bits used) and an election record in two words (26 bits
// and NS * lb bits used).  Every byte of a row is paid three times per distinct state (spec_raft.h), so here
//   * the NS voterLog words share ONE word: server i's field at bit NS * lb * i;
//   * an election record is ONE word: word 0 | word 1 << 26.
// Stored layout:  fp | glob | srv[NS] | voterLog | messages | elections | allLogs   — 13 words instead of 17 for the bench model.
//
// Nothing of the lowering is written twice.  Every function that only READS a row forwards to SpecRaft<NS> through a View: a Ref
// whose get(logical word) returns the field from the packed word, so compute(), load(), the guards and the fingerprint terms are
// the base's own.  The fingerprint hashes logical fields: fingerprints, seen-set behaviour and every count are bit-identical.
// The WRITERS take a concrete WordRef and are written for the packed row (store_row: every word stored once, as the round-5
// writer of spec_raft.h does).  export_row / import_row turn a stored row into the 2 + 2 NS + ... row of SpecRaft<NS> and back:
// that is the row the C ABI hands out and takes, whatever the engine stores.
#pragma once
#include "spec_raft.h"

namespace mc {

template <int NS>
struct SpecRaftPacked : SpecRaft<NS> {
    using B = SpecRaft<NS>;
    using Params = RaftParams;
    using Local = typename B::Local;
    using Delta = typename B::Delta;
    using Guards = typename B::Guards;
    using Summary = typename B::Summary;
    static constexpr bool RAFT_PACKED = true;
    static constexpr int EL_BITS = 26;  // election word 0 of the base: eterm[0,3) eleader[3,6) evotes[6,11) elog[11,26)
    // ---------------------------------------------------------------- word layout (stored)
    static constexpr int P_FP = 0, P_GLOB = 1;
    MC_HD static constexpr int P_SRV(int i) { return 2 + i; }
    static constexpr int P_VL = 2 + NS;
    static constexpr int P_MSG0 = 3 + NS;
    MC_HD static int P_EL0(const Params &p) { return P_MSG0 + B::msg_words(p); }
    MC_HD static int P_ALL0(const Params &p) { return P_MSG0 + B::msg_words(p) + p.ce; }
    MC_HD static int words(const Params &p) { return P_MSG0 + B::msg_words(p) + p.ce + B::all_words(p); }
    static constexpr int MAX_WORDS = B::MAX_WORDS;  // (buffers sized for the base's rows hold these)
    static constexpr int PMAX_WORDS = P_MSG0 + 32 + 8 + 16;
    MC_HD static int vbits(const Params &p) { return NS * p.lb; }  // bits of one server's voterLog field
    MC_HD static bool packable(const Params &p) { return NS * NS * p.lb <= 64 && EL_BITS + NS * p.lb <= 64; }
    MC_HD static int export_words(const Params &p) { return B::words(p); }

    // The read view: get(w) takes a word index of the BASE's layout
    template <class Ref>
    struct View {
        Ref r;
        int vb, nmw, ce;
        uint64_t vmask;   // (1 << vb) - 1
        // ONE load whatever w is: (stored word, shift, mask) are picked by selects — an index that differs from lane to lane (the
        // server a message is for, a message slot) costs a few VALU instructions, no divergent branch; a constant one folds away
        MC_HD uint64_t get(int w) const {
            int phys = w, sh = 0;
            uint64_t mask = ~0ull;
            if (w >= 2 && w < B::W_MSG0) {
                const int i = (w - 2) >> 1;
                const bool vl = ((w - 2) & 1) != 0;
                phys = vl ? P_VL : 2 + i;
                sh = vl ? vb * i : 0;
                mask = vl ? vmask : ~0ull;
            } else if (w >= B::W_MSG0) {
                const int e = w - B::W_MSG0 - nmw;   // < 0: a message word
                const bool el = e >= 0 && e < 2 * ce, hi = (e & 1) != 0;
                phys = e < 0 ? w - (NS - 1) : el ? P_MSG0 + nmw + (e >> 1) : w - (NS - 1) - ce;
                sh = el && hi ? EL_BITS : 0;
                mask = el && !hi ? (1ull << EL_BITS) - 1ull : ~0ull;
            }
            return (r.get(phys) >> sh) & mask;
        }
    };
    template <class Ref>
    MC_HD static View<Ref> view(const Params &p, Ref s) { return View<Ref>{s, vbits(p), B::msg_words(p), p.ce, (1ull << vbits(p)) - 1ull}; }

    // ---------------------------------------------------------------- rows in and out
    static void export_row(const Params &p, const uint64_t *stored, uint64_t *pub) {
        const View<CWordRef> v = view(p, CWordRef{stored, 1});
        for (int w = 0; w < B::words(p); w++) pub[w] = v.get(w);
    }
    // (a bit permutation that drops the bits no field holds: a mask of the public row is imported like a row)
    static void import_row(const Params &p, const uint64_t *pub, uint64_t *stored) {
        const int vb = vbits(p), nmw = B::msg_words(p);
        stored[P_FP] = pub[B::W_FP];
        stored[P_GLOB] = pub[B::W_GLOB];
        uint64_t vl = 0;
        for (int i = 0; i < NS; i++) {
            stored[P_SRV(i)] = pub[B::W_SRV(i)];
            vl |= (pub[B::W_VL(i)] & ((1ull << vb) - 1ull)) << (vb * i);
        }
        stored[P_VL] = vl;
        for (int m = 0; m < nmw; m++) stored[P_MSG0 + m] = pub[B::W_MSG0 + m];
        for (int e = 0; e < p.ce; e++) {
            const uint64_t *ew = pub + B::W_EL0(p) + e * B::EL_WORDS;
            stored[P_EL0(p) + e] = (ew[0] & ((1ull << EL_BITS) - 1ull)) | ((ew[1] & ((1ull << vb) - 1ull)) << EL_BITS);
        }
        for (int a = 0; a < B::all_words(p); a++) stored[P_ALL0(p) + a] = pub[B::W_ALL0(p) + a];
    }

    // ---------------------------------------------------------------- readers: the base's, through the view
    template <class Ref>
    MC_HD static void stage_range(const Params &, Ref s, int &lo, int &n) { lo = P_MSG0; n = (B::g_nm(s.get(P_GLOB)) + 1) >> 1; }
    template <class Ref> MC_HD static uint64_t rd_msg(Ref s, int k) { return (s.get(P_MSG0 + (k >> 1)) >> (32 * (k & 1))) & 0xffffffffull; }
    template <class Ref>
    MC_HD static uint64_t fp_of(const Params &, Ref s) { return fp_nonzero(s.get(P_FP)); }
    template <class Ref>
    MC_HD static uint64_t fp_recompute(const Params &prm, Ref s) { return B::fp_recompute(prm, view(prm, s)); }
    template <bool WANT_FP = true, class Ref>
    MC_HD static void load(const Params &prm, Ref s, Local &l) { B::template load<WANT_FP>(prm, view(prm, s), l); }
    template <class Ref>
    MC_HD static void load_expand(const Params &prm, Ref s, Local &l, Guards &g) { B::load_expand(prm, view(prm, s), l, g); }
    template <bool MEM = false, int FAM = -1, class Ref>
    MC_HD static unsigned compute(const Params &prm, const Local &l, Ref s, int slot, Delta &d, int &action) {
        return B::template compute<MEM, FAM>(prm, l, view(prm, s), slot, d, action);
    }
    template <class Ref>
    MC_HD static bool message_generated_only(const Params &prm, const Local &l, Ref s, int slot) {
        const int q = slot - B::FIX, k = q / 3;
        return q % 3 == 1 && l.inflight >= prm.max_msgs && k < l.nm && B::m_count(rd_msg(s, k)) == 1;
    }
    template <int FAM, class Ref>
    MC_HD static unsigned eval_pair(const Params &prm, const Summary &q, Ref s, int slot, uint64_t &fp) {
        return B::template eval_pair<FAM>(prm, q, view(prm, s), slot, fp);
    }
    template <class Ref>
    MC_HD static unsigned eval(const Params &prm, Local &l, Ref s, int slot, uint64_t &fp) { return B::eval(prm, l, view(prm, s), slot, fp); }
    // (eval_dense, guards, parent_status, init_status, summarize and the Guards helpers read no row: the base's as they are)

    // ---------------------------------------------------------------- Init
    MC_HD static void init(const Params &prm, uint64_t, WordRef out) {
        for (int w = 0; w < words(prm); w++) out.set(w, 0);
        const uint64_t sv = B::sv_reset_leader_vars(B::sv_set_term(0, 1), 1);
        for (int i = 0; i < NS; i++) out.set(P_SRV(i), B::pack_srv(sv, 0));
        out.set(P_GLOB, B::pack_glob(1, 0));
        out.set(P_FP, B::hheader(prm, view(prm, out)));
    }

    // ---------------------------------------------------------------- writers
    // EVERY WORD IS STORED ONCE (spec_raft.h, round 5): the action has been evaluated — through the view — and its handful of changes
    // wait in the Delta; the row is copied through them.  `s` is the STORED parent row; of `l` the writer reads nm, glob, nadd and
    // addmask (a Local made by load() or from a Summary).  ok = false writes the parent itself.
    template <class Ref>
    MC_HD static void store_row(const Params &prm, const Local &l, Ref s, const Delta &d, bool ok, uint64_t nfp, WordRef out) {
        const int W = words(prm);
        const uint64_t nglob = ok ? B::pack_glob(d.glob, d.clog) : 0ull;
        const int srv = ok ? d.srv : -1;
        const uint64_t nsrv = srv >= 0 ? B::pack_srv(d.sv, d.log) : 0ull;
        // the voterLog word: the parent's with server srv's field cleared (vmode 1) or with entry (srv, vj) OR-ed in (vmode 2: the entry was empty)
        // (kept as a mode, a shift and the 13-bit log until the word passes: three registers)
        const int vb = vbits(prm);
        const int vm = srv >= 0 ? d.vmode : 0, vsh = vb * srv + (vm == 2 ? prm.lb * d.vj : 0);
        const uint32_t vlog = (uint32_t)d.vlog;
        // the one or two message slots the action rewrites (both may share a word)
        const int wa = d.midxA >> 1, wb = d.midxB >> 1;
        bool hasA = false, hasB = false;
        uint64_t xa = 0, xb = 0;
        if (ok && (d.nmop & 1)) {
            xa = 2 * wa < l.nm ? s.get(P_MSG0 + wa) : 0ull;
            xa = B::set_half(xa, d.midxA, d.mnewA);
            if ((d.nmop & 2) && wb == wa) xa = B::set_half(xa, d.midxB, d.mnewB);
            hasA = true;
        }
        if (ok && (d.nmop & 2) && !((d.nmop & 1) && wb == wa)) { xb = B::set_half(s.get(P_MSG0 + wb), d.midxB, d.mnewB); hasB = true; }
        const int nmw = B::msg_words(prm), wel = P_MSG0 + nmw, wall = wel + prm.ce;
        const int e0 = ok && d.eadd ? B::g_ne(l.glob) : -1;   // an appended election is one word
        // allLogs' additions (the same for every successor of this parent) land in slots na, na + 1, ...: at most NS of them, 4 per word
        constexpr int ALLW = (NS + 3) / 4 + 1;
        int qlo = 0, qhi = -1;
        uint64_t xall[ALLW];
#pragma unroll
        for (int j = 0; j < ALLW; j++) xall[j] = 0;
        if (ok && l.nadd) {
            const int na = B::g_na(l.glob);
            qlo = na >> 2;
            qhi = (na + l.nadd - 1) >> 2;
            if (qhi >= B::all_words(prm)) qhi = B::all_words(prm) - 1;
#pragma unroll
            for (int j = 0; j < ALLW; j++) {
                const int qq = qlo + j;
                if (qq <= qhi) {
                    uint64_t x = qq * 4 < na ? s.get(wall + qq) : 0ull;
                    int pos = na;
#pragma unroll
                    for (int i = 0; i < NS; i++)
                        if (l.addmask >> i & 1) {
                            if (pos < prm.ca && (pos >> 2) == qq) x |= (s.get(P_SRV(i)) >> B::LOGSH) << (16 * (pos & 3));
                            pos++;
                        }
                    xall[j] = x;
                }
            }
        }
        // (groups of COPY words, all asked for before the first is used: the bench rows are one group)
        constexpr int COPY = 14;
        uint64_t t[COPY];
#pragma unroll
        for (int w0 = 0; w0 < PMAX_WORDS; w0 += COPY) {
            if (w0 < W) {
#pragma unroll
                for (int u = 0; u < COPY; u++) t[u] = s.get(w0 + u < W ? w0 + u : W - 1);
#pragma unroll
                for (int u = 0; u < COPY; u++) {
                    const int w = w0 + u;   // (a compile-time constant after unrolling)
                    if (w >= W) continue;
                    uint64_t v = t[u];
                    if (w == P_FP) { if (ok) v = nfp; }
                    else if (w == P_GLOB) { if (ok) v = nglob; }
                    else if (w < P_VL) { if (srv == w - 2) v = nsrv; }
                    else if (w == P_VL) {
                        if (vm == 1) v &= ~(((1ull << vb) - 1ull) << vsh);
                        if (vm == 2) v |= (uint64_t)vlog << vsh;
                    }
                    else {
                        const int mw = w - P_MSG0;
                        if (mw < nmw) {
                            if (hasA && wa == mw) v = xa;
                            if (hasB && wb == mw) v = xb;
                        } else if (w < wall) {
                            if (w - wel == e0) v = d.ew.get(0) | (d.ew.get(1) << EL_BITS);
                        } else {
                            const int qq = w - wall;
#pragma unroll
                            for (int j = 0; j < ALLW; j++) if (qq == qlo + j && qq <= qhi) v = xall[j];
                        }
                    }
                    out.set(w, v);
                }
            }
        }
    }
    // re-evaluate `slot` on parent `s` and write the whole successor to `out` (k_materialise, walks, traces); a pair that is no
    // successor writes the parent itself, as the base does
    template <bool KNOWN, class Ref>
    MC_HD static unsigned apply_eval_store(const Params &prm, Ref s, int slot, uint64_t fp_known, WordRef out) {
        prefetch_row(s, words(prm));   // (load() walks the bag and allLogs in dependent rounds: after this pass they hit the CU's L1)
        const View<Ref> v = view(prm, s);
        Local l;
        B::template load<!KNOWN>(prm, v, l);
        Delta d;
        int action;
        const unsigned st = B::template compute<true>(prm, l, v, slot, d, action);
        const bool ok = (st & ST_ENABLED) && !(st & (ST_OVERFLOW | ST_SPECERR));
        const uint64_t nfp = !ok ? 0ull : KNOWN ? fp_known : B::delta_fp(prm, l, v, d);
        store_row(prm, l, s, d, ok, nfp, out);
        return st;
    }
    template <class Ref>
    MC_HD static unsigned apply(const Params &prm, Ref s, int slot, WordRef out) { return apply_eval_store<false>(prm, s, slot, 0, out); }
    template <class Ref>
    MC_HD static unsigned apply_known_fp(const Params &prm, Ref s, int slot, uint64_t fp_nz, WordRef out) {
        if (fp_nz == fp_nonzero(0)) return apply_eval_store<false>(prm, s, slot, 0, out);
        return apply_eval_store<true>(prm, s, slot, fp_nz, out);
    }
    // the in-wave writer: what the parent's lane derived from the row lies in LDS (Summary)
    template <class Ref>
    MC_HD static unsigned apply_summary_patch(const Params &prm, const Summary &q, Ref s, int slot, uint64_t fp_nz, WordRef out) {
        const View<Ref> v = view(prm, s);
        Local l;
        B::template local_of_summary<-1>(q, v, l);
        Delta d;
        int action;
        const unsigned st = B::template compute<true>(prm, l, v, slot, d, action);
        const bool ok = (st & ST_ENABLED) && !(st & (ST_OVERFLOW | ST_SPECERR));  // (false: never the case for a survivor)
        // the fingerprint arrives with the survivor; the one ambiguous value (raw sum 0 or the substitute itself) is recomputed
        const uint64_t nfp = !ok ? 0ull : fp_nz != fp_nonzero(0) ? fp_nz : B::delta_fp(prm, l, v, d);
        store_row(prm, l, s, d, ok, nfp, out);
        return st;
    }

    // ---------------------------------------------------------------- host side: names and text, over the exported row
    static int action_of(const Params &prm, const uint64_t *parent, int slot) {
        uint64_t pub[B::MAX_WORDS];
        export_row(prm, parent, pub);
        return B::action_of(prm, pub, slot);
    }
    static int format(const Params &prm, const uint64_t *w, char *buf, size_t cap) {
        uint64_t pub[B::MAX_WORDS];
        export_row(prm, w, pub);
        return B::format(prm, pub, buf, cap);
    }
};

}  // namespace mc
