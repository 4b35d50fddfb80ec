// spec_vm_cfg.h — cfg ACTION_CONSTRAINT and VIEW for the interpreter of compiled PlusCal programs: SpecVmCfgT is
// SpecVmT (spec_vm.h: the interpreter itself, its opcodes and its rows, all unchanged) with the two statements folded into the status
// `step` returns and into the fingerprint.  This is the lowering the engine and the host builds run for MC_SPEC_PCAL (spec_registry.h,
// engine.hip); for a program without the statements it computes what SpecVmT computes.
//
// Where the entries live.  Neither the VMH_* header nor VmParams has room for them (both are pinned: a program without the statements
// keeps its image, its parameters and its checkpoint identity), so they sit in a table of VMX_SIZE words BEHIND the image, at
// code[code_len ..): always there, all zero without the statements.  Every lane reads the same words of it: the branches on the two
// counts are wave-uniform.  Component k of the view: view_n > 0: the cells view_a .. view_a + view_n - 1; view_n == 0: the value of the
// code at view_a.
//
// How a primed variable is read, without a new opcode.  The interpreter has two read sources: v at "old" depth 0, `old` inside
// VM_OLD_ON .. VM_OLD_OFF.  The code of an action constraint stores nothing, so it runs with v = the state being EXPANDED and
// old = the SUCCESSOR: pcal_compile.cpp emits its body at depth 0 (definitions are inlined without the VM_OLD_ON they get elsewhere)
// and wraps exactly the access to a primed variable in VM_OLD_ON / VM_OLD_OFF.
#pragma once
#include "spec_vm.h"

namespace mc {

constexpr int VM_MAX_ACON = 4, VM_MAX_VIEW = 16;   // action constraints / view components per cfg (pcal_compile.cpp refuses more)
enum VmExt : int32_t { VMX_NACON = 0, VMX_NVIEW, VMX_ACON0, VMX_VIEW_A0 = VMX_ACON0 + VM_MAX_ACON, VMX_VIEW_N0 = VMX_VIEW_A0 + VM_MAX_VIEW, VMX_SIZE = VMX_VIEW_N0 + VM_MAX_VIEW };
MC_HD const int32_t *vm_ext(const VmParams &p) { return p.code + p.code_len; }
// The safety parts of the cfg's PROPERTYs: the action properties `[][A]_v` (compiled as `A \/ UNCHANGED v`, an action
// constraint's kind of code) and the initial predicates.  The table above has no spare word and may not grow (a program without them keeps
// its image), so their counts share the word of the action constraints' count — bits 8..15 and 16..23 of it, zero without them — and their
// entries FOLLOW the table: VMX_SIZE + k, the initial predicates' behind the action properties'.  (`[]P` is an invariant entry of the header.)
constexpr int VM_MAX_APROP = 8;
MC_HD int vm_nacon(const int32_t *x) { return x[VMX_NACON] & 0xff; }
MC_HD int vm_naprop(const int32_t *x) { return x[VMX_NACON] >> 8 & 0xff; }
MC_HD int vm_ninitp(const int32_t *x) { return x[VMX_NACON] >> 16 & 0xff; }
MC_HD int vm_ext_words(const VmParams &p) { const int32_t *x = vm_ext(p); return VMX_SIZE + vm_naprop(x) + vm_ninitp(x); }

template <int MAXV>
struct SpecVmCfgT : SpecVmT<MAXV> {
    using Base = SpecVmT<MAXV>;
    using Params = VmParams;
    using Local = typename Base::Local;
    static constexpr int MAX_VARS = Base::MAX_VARS;
    using Base::R_OK;

    // cfg VIEW: the fingerprint of the view's values and of nothing else — the values in the order of the view's components, two per word,
    // in fp_vals' form (what generated code with the interpreter's rows computes too); false = an evaluation error inside a component
    // (the value hashed in its place is a fixed one: fp_of has no status to return)
    MC_HD static bool fp_view(const Params &p, int32_t *v, uint64_t &fp) {
        uint64_t h = 0x9e3779b97f4a7c15ull, word = 0;
        int n = 0;   // values so far
        bool ok = true;
        auto put = [&](int32_t x) {
            if (n & 1) h = fmix64(h ^ ((word | (uint64_t)(uint32_t)x << 32) + 0x632be59bd9b4e019ull * (uint64_t)(n / 2 + 1)));
            else word = (uint64_t)(uint32_t)x;
            ++n;
        };
        const int32_t *x = vm_ext(p);
        for (int k = 0; k < x[VMX_NVIEW]; ++k) {
            const int32_t a = x[VMX_VIEW_A0 + k], cells = x[VMX_VIEW_N0 + k];
            if (cells > 0) {
                for (int i = 0; i < cells; ++i) put(v[a + i]);
            } else {
                int32_t res;
                int aux;
                if (Base::run(p, a, 0, 0, 0, v, res, aux) != R_OK) { ok = false; res = VM_DEFAULT_INIT; }
                put(res);
            }
        }
        if (n & 1) h = fmix64(h ^ (word + 0x632be59bd9b4e019ull * (uint64_t)(n / 2 + 1)));
        fp = fp_nonzero(h);
        return ok;
    }
    // cfg ACTION_CONSTRAINT: the transition cur -> v outside one of them is treated as a successor outside a CONSTRAINT (ST_OUT_OF_MODEL).
    // (the code reads, never stores: `cur` is its v, the successor its `old` — see the head of this file)
    MC_HD static unsigned acon_status(const Params &p, const int32_t *cur, const int32_t *v) {
        const int32_t *x = vm_ext(p);
        for (int k = 0; k < vm_nacon(x); ++k) {
            int32_t res;
            int aux;
            const int r = Base::run(p, x[VMX_ACON0 + k], 0, 0, 0, const_cast<int32_t *>(cur), res, aux, v);
            if (r != R_OK) return ST_SPECERR;
            if (!res) return ST_OUT_OF_MODEL;
        }
        return 0;
    }
    // A PROPERTY's `[][A]_v` on the step cur -> v (TLC's doNextCheckImplied): property k broken = ST_INVARIANT with the index ninv + k, behind
    // the invariants' (the `[]P` entries among them).  The code is an action constraint's: `cur` is its v, the successor its `old`.
    MC_HD static unsigned aprop_status(const Params &p, const int32_t *cur, const int32_t *succ) {
        const int32_t *x = vm_ext(p);
        for (int k = 0; k < vm_naprop(x); ++k) {
            int32_t res;
            int aux;
            const int r = Base::run(p, x[VMX_SIZE + k], 0, 0, 0, const_cast<int32_t *>(cur), res, aux, succ);
            if (r != R_OK) return ST_SPECERR;
            if (!res) return ST_INVARIANT | (unsigned)(p.ninv + k) << 8;
        }
        return 0;
    }
    // a PROPERTY's initial predicates on an initial state, indices behind the action properties'
    MC_HD static unsigned initp_status(const Params &p, int32_t *v) {
        const int32_t *x = vm_ext(p);
        const int np = vm_naprop(x);
        for (int k = 0; k < vm_ninitp(x); ++k) {
            int32_t res;
            int aux;
            if (Base::run(p, x[VMX_SIZE + np + k], 0, 0, 0, v, res, aux) != R_OK) return ST_SPECERR;
            if (!res) return ST_INVARIANT | (unsigned)(p.ninv + np + k) << 8;
        }
        return 0;
    }

    MC_HD static uint64_t fp_of(const Params &p, CWordRef s) {
        int32_t v[MAX_VARS];
        Base::unpack(p, s, v);
        if (vm_ext(p)[VMX_NVIEW]) { uint64_t fp; (void)fp_view(p, v, fp); return fp; }
        return Base::fp_vals(p, v);
    }
    MC_HD static unsigned init_status(const Params &p, CWordRef s) {
        int32_t v[MAX_VARS];
        Base::unpack(p, s, v);
        uint64_t fp;
        if (vm_ext(p)[VMX_NVIEW] && !fp_view(p, v, fp)) return ST_ENABLED | ST_SPECERR;
        unsigned st = Base::inv_status(p, v);
        if (vm_ninitp(vm_ext(p)) && !(st & (ST_INVARIANT | ST_SPECERR))) st |= initp_status(p, v);   // (an INVARIANT comes first: the word carries one index)
        return ST_ENABLED | st;
    }
    // SpecVmT::step, then the action constraints: never on the terminating disjunct (it reaches no code), never on a successor that is
    // an error or outside a CONSTRAINT already
    MC_HD static unsigned step(const Params &p, const int32_t *cur, int slot, int32_t *v) {
        unsigned st = Base::step(p, cur, slot, v);
        const int32_t *x = vm_ext(p);
        if (!x[VMX_NACON] || !(st & ST_ENABLED) || slot == p.ninst * p.maxch) return st;
        // the action properties: every generated successor, outside a CONSTRAINT or not, stored before or not; an INVARIANT it breaks as
        // well is what is reported
        unsigned ap = 0;
        if (vm_naprop(x) && !(st & (ST_SPECERR | ST_ASSERT | ST_OVERFLOW | ST_INVARIANT))) ap = aprop_status(p, cur, v);
        if (vm_nacon(x) && !(st & (ST_SPECERR | ST_OUT_OF_MODEL | ST_ASSERT | ST_OVERFLOW)))
            st |= acon_status(p, cur, v);
        if (!(st & ST_SPECERR)) st |= ap;   // (a refused step is checked too; an evaluation error of the constraint is the error)
        return st;
    }
    template <class Ref>
    MC_HD static unsigned eval(const Params &p, const Local &l, Ref, int slot, uint64_t &fp) {
        int32_t v[MAX_VARS];
        const unsigned st = step(p, l.v, slot, v);
        if (st & ST_ENABLED) {
            if (vm_ext(p)[VMX_NVIEW]) { if (!fp_view(p, v, fp)) return ST_ENABLED | ST_SPECERR; }
            else fp = Base::fp_vals(p, v);
        }
        return st;
    }
    template <class Ref>
    MC_HD static unsigned apply(const Params &p, Ref s, int slot, WordRef out) {
        int32_t cur[MAX_VARS], v[MAX_VARS];
        Base::unpack(p, s, cur);
        const unsigned st = step(p, cur, slot, v);
        for (int w = 0; w < p.words; ++w) out.set(w, Base::pack(v, w, p.nv));
        return st;
    }
};
using SpecVmCfg = SpecVmCfgT<128>;   // what MC_SPEC_PCAL runs (spec_registry.h, engine.hip): the widest instantiation and the narrower ones
using SpecVmCfg16 = SpecVmCfgT<16>;
using SpecVmCfg32 = SpecVmCfgT<32>;
using SpecVmCfg64 = SpecVmCfgT<64>;

}  // namespace mc
