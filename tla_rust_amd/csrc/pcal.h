// pcal.h — PlusCal front-end (p-syntax): parser, pcal2tla-style translator, compiler to the bytecode of
// spec_vm.h.  Host only.
//
// The reference keeps its two root specs UNtranslated (pcal_intro.tla:4-19, atomic_add.tla:4-23) and its
// Makefile runs `pcal2tla *tla` before `tlc *tla` (Makefile:3-7).  This is the `transpile` half: the
// translation follows examples/p-manual.pdf §3.8 and App. B (one action per label guarded by pc[self],
// `await` as an enabling conjunct, Assert(...) with the source position, the terminating disjunct), in the
// layout of the translator whose output the README quotes (action spans README.md:278-318).
#pragma once
#include <memory>
#include <string>
#include <vector>

namespace pcal {

struct Pos { int line = 0, col = 0; };

struct Expr;
using EP = std::shared_ptr<Expr>;
struct Expr {
    enum K { NUM, STR, BOOL, ID, UNOP, BINOP, INDEX, IF, QUANT, SETENUM, TUPLE, FUNCDEF, PRIME, CALL, RECORD, DOT, SETOF } k = NUM;
    long long num = 0;      // NUM, BOOL
    std::string s;          // ID name, STR text, operator text, QUANT "\\A" / "\\E", CALL operator name, DOT field name
    std::string bound;      // QUANT / FUNCDEF / SETOF bound variable (SETOF: s = "filter" {x \in S : P} or "map" {e : x \in S}; a = [domain, P or e])
    std::vector<EP> a;      // operands; INDEX: [fn, index]; IF: [c, t, e]; QUANT / FUNCDEF: [domain, body]; DOT: [record]; RECORD: the values
    std::vector<std::string> names;  // RECORD [f |-> e, g |-> h]: the field names, in the order written
    bool paren = false;     // written inside ( )
    Pos pos;
};

struct Stmt;
using SP = std::shared_ptr<Stmt>;
struct Stmt {
    enum K { ASSIGN, IF, WHILE, EITHER, WITH, AWAIT, ASSERT, SKIP, GOTO, PRINT, CALL, RETURN } k = SKIP;
    std::string label;                     // "" = unlabeled
    char fair_mod = 0;                     // the label's fairness modifier: '+' (`l:+`), '-' (`l:-`) or 0
    std::string in_proc, src_label;        // a statement of a procedure's body copied into a process (expand_procedures): the procedure,
                                           // and the label as the procedure wrote it (every copy of `l` is one action l(self) of pcal2tla)
    Pos pos;                               // of the statement keyword / lhs (asserts print it)
    std::string var;                       // ASSIGN lhs, WITH variable, GOTO target
    EP idx;                                // ASSIGN lhs index (x[i] := e), may be null
    std::string field;                     // ASSIGN lhs field path (r.f := e, r[i].f := e, r.f.g := e: "f.g"); gone after flatten_records
    std::string whole;                     // ASSIGN to a variable that flatten_records made from the record variable `whole`
    EP e;                                  // ASSIGN rhs; condition of IF / WHILE / AWAIT / ASSERT; WITH set or value
    bool with_eq = false;                  // with x = e
    std::vector<std::vector<SP>> blocks;   // IF: then, else; EITHER: branches; WHILE / WITH: body
    std::vector<SP> more;                  // ASSIGN: the other assignments of `a := e || b := f` (all right-hand sides
                                           // see the values before the statement)
    std::vector<EP> args;                  // CALL: the arguments (`var` = the procedure's name); gone after expand_procedures
};

struct VarDecl {
    std::string name;
    bool in_set = false;   // `x \in S` instead of `x = e`
    bool no_init = false;  // `variable x;`: the translation initialises it to the model value defaultInitValue
    EP init;
    Pos pos;
};

struct Proc {
    std::string name;
    bool is_set = false;   // process P \in S   vs   process P = e
    int fair = 0;          // 0 = `process`, 1 = `fair process` (weak fairness), 2 = `fair+ process` (strong)
    bool label_mods = false;   // some label of the body carries a `+` / `-` modifier (Stmt::fair_mod; kept here too: the passes that
                               // rebuild statements — records, procedures — keep a label's name only)
    EP id;
    std::vector<VarDecl> locals;
    std::vector<SP> body;
};

// procedure P(a, b = e) variables x = e; begin ... return; end procedure   (p-manual section 3.5)
struct Procedure {
    std::string name;
    std::vector<VarDecl> params;   // `a` (initially defaultInitValue) or `a = e`
    std::vector<VarDecl> locals;   // (re)initialised on every call
    std::vector<SP> body;
    Pos pos;
};

// A variable whose initial value is a record constructor (or a function to records): kept FIELD BY FIELD (flatten_records, pcal.cpp).
struct RecordVar {
    std::string name;                  // r: the variables of the translation are r_f, one per field
    std::vector<std::string> fields;
    bool array = false;                // r = [x \in S |-> [f |-> e, ...]]
    bool seq = false;                  // a SEQUENCE of records (q = <<>> ... Append(q, [f |-> e, ...]); with `array`: [x \in S |-> <<>>], the
                                       // channels of a message-passing algorithm): one sequence per field, all of the same length
    std::string bound;                 // array: x
    EP domain;                         // array: S
    bool set = false;                  // a SET of records (msgs = {} ... msgs := msgs \cup {[type |-> "1a", bal |-> b]}): stays ONE set-valued variable of the
                                       // translation (as pcal2tla keeps it); the compiled program keeps its elements sorted, field by field
    EP shape;                          // seq / set: the constructor that says which fields (and of which types) an element has
    int proc = -1;                     // index into Module::procs of the process it is local to, -1 = global
    std::vector<std::string> sub;      // the fields that are records themselves (nested records): r_f is a RecordVar of depth + 1
    int depth = 0;                     // 0 = a variable of the algorithm, k = a field of a record of depth k - 1
};

struct Definition {
    std::string name;
    std::vector<std::string> params;
    EP body;
    int line = 0;
    bool in_define = false;   // from the algorithm's `define` block (printed in the translation)
};
// A definition of the module that is no state-level expression but a temporal formula: kept so that a cfg PROPERTY
// that names it can be classified.  items: the conjuncts of an accepted body, each one of the four shapes under its bounded `\A`s.
struct LiveItem {
    int kind = 0;                                       // 0 `A ~> B`, 1 `[]<>B`, 2 `<>B`, 3 `<>[]A` (MC_LIVE_* of tlamc.h)
    std::vector<std::pair<std::string, EP>> quants;     // the `\A x \in S :` around it, outermost first: (x, S)
    EP a, b;                                            // the state predicates (null where the shape has none)
    std::string a_text, b_text;                         // their tokens, joined by one blank: what predicates are deduplicated by
};
// A SAFETY conjunct of such a definition: `[][A]_v`, `[]P` or an initial predicate.  What is checked is one Boolean
// expression, kept as the body of a definition of the module under a name no module text can write (`def`): `A \/ UNCHANGED v` with its
// bounded `\A`s inside for a step, P, or I.  Being a definition, it goes through the record flattener with every other one.
struct SafetyItem {
    int kind = 0;                                       // 0 `[][A]_v` (a property of a step), 1 `[]P`, 2 an initial predicate (MC_APROP_* of tlamc.h)
    std::string def, text;                              // the definition that holds the expression; the conjunct as written
    EP body;                                            // (until parse_module has made the definition)
};
struct TemporalDef {
    std::string name;
    int line = 0;
    std::vector<LiveItem> items;
    std::vector<SafetyItem> safety;
    std::vector<std::pair<std::string, std::string>> named;   // conjuncts beside a `[][A]_v` that are neither (WF_ / SF_): (text, why); the liveness items are
                                                              // then refused with them — they would be checked under another fairness than the property's
    std::string refusal;                                // "" = accepted; else why the body is none of the accepted shapes
    std::string safety_error;                           // a `[][A]_v` / `<<A>>_v` whose form is refused (a compile error for the cfg that names it)
};
struct Macro {
    std::string name;
    std::vector<std::string> params;
    std::vector<SP> body;
};

struct Module {
    std::string name;
    std::string algorithm;
    bool fair_algorithm = false;            // `--fair algorithm`: every process is (weakly) fair; a uniprocess one gets WF_vars(Next)
    std::vector<std::string> constants;     // CONSTANT(S) declared by the module
    std::vector<VarDecl> globals;
    std::vector<Proc> procs;                // a uniprocess algorithm is one Proc with an empty name
    std::vector<Definition> defs;           // definitions of the `define` block and of the module around the algorithm
    std::vector<std::pair<std::string, std::string>> dropped_defs;   // definitions of the module text beyond the record subset: (name, why), for the
                                            // message of a cfg statement that names one (VIEW, ACTION_CONSTRAINT)
    std::vector<TemporalDef> temporal;      // the definitions beyond the expression subset: temporal formulas, accepted or refused
    std::vector<Macro> macros;
    std::vector<Procedure> procedures;      // as written; expand_procedures() has inlined them into the processes' bodies
    bool had_procedures = false;
    std::vector<RecordVar> records;         // record variables, replaced by their fields' variables in globals / locals
    int alg_first_line = 0, alg_last_line = 0;   // lines of "(* --algorithm" and "end algorithm *)"
    bool has_translation = false;
    int tr_first_line = 0, tr_last_line = 0;     // "\* BEGIN TRANSLATION" .. "\* END TRANSLATION"
};

// Parse the PlusCal algorithm (and the definitions around it) of a module text.  Returns "" or an error message.
// PROCEDURES (round 4): parsed and then EXPANDED into the calling processes — every call site gets its own copy of the procedure's
// body (labels `Label_pK`, K = the number of the copy), `call` becomes "parameters := arguments || locals := their initial values;
// goto the copy's first label" and `return` "parameters, locals := their initial values; goto the label after the call", all in
// the step the statement was in.  For NON-RECURSIVE procedures this is a bijection on states with the translation pcal2tla gives
// (pc + the contents of `stack` <-> the copy's pc; a frame's saved values are the initial values, which `return` restores), so
// distinct / generated / depth and every verdict agree (tests/test_pcal.py checks it against hand-written stack translations);
// what differs is the TEXT of the translation and of a printed state: no `stack` variable, the copies' label names.
// `call P(..); return` (pcal2tla's tail call) is refused with a message.
// RECURSIVE procedures (round 5; a procedure that can reach itself through `call`, mutual recursion included) get ONE copy of the body per
// calling process and a BOUNDED call stack per procedure, kept as plain variables: the depth counter P_sp, and for every level
// K = 1 .. D (D = $TLAMC_PCAL_STACK, default 4) the return-site code P_retK and one slot vK per parameter / procedure variable v — what a
// frame of pcal2tla's `stack` holds (the return pc and the values the procedure's variables had BEFORE the call).  `call`: assert
// P_sp < D (a run that needs a deeper stack fails THERE, with the call's position, instead of being cut short silently), fill level
// P_sp + 1, parameters := arguments, locals := initial values, goto the body's first label; `return`: branch on the top frame's
// return-site code, restore the variables from it, put the frame back to its initial values (two states must not differ in what lies
// above the stack), pop, goto the site.  pc + `stack` <-> pc + (P_sp, frames) is again a bijection on states — the return sites tell
// how the per-procedure stacks interleave — so counts, depth and verdicts equal those of pcal2tla's translation for every run that
// stays within D frames (tests/test_pcal.py: the hand-written stack translation tests/golden/pcal_recursion/RecursiveSumStack.tla).
// RECORDS (round 4): a variable initialised with `[f |-> e, g |-> h]` (or `[x \in S |-> [f |-> e, ...]]`) is kept field by field —
// variables r_f, r_g; `r.f` / `r[i].f` read them, `r.f := e` / `r[i].f := e` assign one, `r := [f |-> a, g |-> b]`, `r := s`
// (s another record variable or an element of a record array) assign all fields at once (`||`), `r = s` / `r # s` compare
// fieldwise.  A record value <-> the tuple of its fields is a bijection on states, so counts, depth and verdicts equal those of
// pcal2tla's translation (which keeps r one record-valued variable: tests/test_pcal.py checks it against hand-written record
// translations); the translation's TEXT differs: it declares r_f, r_g and defines `r == [f |-> r_f, g |-> r_g]` after them, so
// that the text around the algorithm (invariants written with r.f) keeps its meaning.  NESTED records (round 5): a field may itself
// be a record; the flattener works one level per pass (r -> r_f -> r_f_g), `r.f.g := e` carries its path in Stmt::field ("f.g"), an
// inner record is assigned / compared leaf by leaf, the translation defines every level, inner before outer.  Refused with a message:
// a record as a whole value anywhere else (`with` over a record, procedure arguments).  SEQUENCES of records (and arrays of them: channels)
// are kept as one sequence per field; a SET of records (a message soup) stays one set-valued variable of the translation and is kept as
// sorted cells by the compiled program (RecordVar::seq / ::set below).
std::string parse_module(const std::string &text, Module &out);

// The text `pcal2tla` inserts: from "\* BEGIN TRANSLATION" to "\* END TRANSLATION" inclusive, '\n' terminated.
// Fairness label by label: the conjuncts pcal2tla gives one process — its own (the labels of its body, without the
// copies of procedure bodies), one per procedure it reaches, one SF per `+` label of a weakly fair process (all copies of the label
// together) — as sets of the translation's labels; empty for an unfair process.  minus: the `-` labels among `labels`, restricted away.
// whole: the process's own conjunct when it reaches no procedure: the action is the process's (P(self), Next), not a disjunction.
struct FairGroup { bool strong = false, whole = false; std::string section, plus; std::vector<std::string> labels, minus; };
struct FairLabel { std::string label, section, src; char mod = 0; };
std::vector<FairLabel> fair_labels(const Proc &p);
std::vector<FairGroup> fairness_groups(const Module &m, const Proc &p);
// act: the process's action; pc: its pc cell; suffix: "(self)" / "(<id>)" / "" after a label's name
std::string fair_group_text(const FairGroup &g, const std::string &act, const std::string &pc, const std::string &suffix);
// label_fair: Spec's fairness conjuncts as pcal2tla writes them for `+` / `-` labels instead of one per process
std::string translate(const Module &m, bool label_fair = false);

// The whole module with the translation inserted after the algorithm comment (replacing an existing one).
std::string transpile_text(const std::string &text, const Module &m, bool label_fair = false);

// ------------------------------------------------------------------------------------------------
// Compilation to the stack machine of spec_vm.h.
struct ConstVal {
    enum K { INT, STR, SET } k = INT;
    long long i = 0;
    std::string s;                 // STR: a string or a model value (both become interned strings)
    std::vector<ConstVal> elems;   // SET
};
struct Config {
    std::vector<std::string> invariants;                       // INVARIANT names, in cfg order
    std::vector<std::string> constraints;                      // CONSTRAINT names
    std::vector<std::pair<std::string, ConstVal>> constants;   // CONSTANT name = value
    std::vector<std::string> properties;                       // PROPERTY names other than Termination, in cfg order (Program::live_props)
    std::vector<std::string> action_constraints;               // ACTION_CONSTRAINT names, in cfg order
    std::string view;                                          // VIEW name, or ""
};

struct VarInfo {
    std::string name;
    bool array = false;       // a function over `ids` (flattened to consecutive variables)
    int base = 0;             // index of the first 32-bit variable
    std::vector<long long> ids;  // domain of the array (process ids for pc and process locals)
    char type = 'i';          // 'i' integer, 'b' boolean, 's' interned string (of the elements for array / seq)
    bool set = false;         // a set of naturals 0..31 (or of interned strings), one cell holding the 32-bit mask
    bool seq = false;         // a bounded sequence: cell `base` = Len, then `cap` element cells
    bool defval = false;      // declared without an initial value: a cell holding VM_DEFAULT_INIT prints as defaultInitValue
    int cap = 0;
    bool rset = false;        // a SET of records: cell `base` = the number of elements, field f of element i at base + 1 + f * cap + i (sorted, spec_vm.h VM_RSADD)
    std::vector<std::string> fields;   // rset: the field names, in the order of the cells
    std::string ftypes;                // rset: their types ('i' / 'b' / 's')
};

struct Program {
    int magic = 0x70634c31;
    std::vector<int> image;               // what the device reads (header, tables, code)
    std::vector<VarInfo> vars;            // VARIABLES order: globals, pc, process locals
    std::vector<std::string> strings;     // interned strings; the first `nlabels` are the labels, "Done" included
    int nlabels = 0, nv = 0, ninst = 0, maxch = 1, pc_base = 0;
    bool multi = true;
    unsigned long long num_init = 1;
    std::vector<std::string> invariants;
    struct AssertPos { int line, col; };
    std::vector<AssertPos> asserts;
    std::string module, translated;       // module name; the module text with the translation inserted
    // fairness (liveness.h): bit k = process instance k (the slot order: slot / maxch) is weakly fair
    unsigned long long fair_mask = 0;
    std::string live_refusal;             // "" = `Termination` can be checked on the state graph; else why not
    // the same for the strong checks: the `fair+` instances among fair_mask's, and the refusal with `fair+` allowed
    unsigned long long strong_mask = 0;
    std::string live_refusal_strong;
    // fairness label by label: pcal2tla's conjuncts exactly.  unit_of[inst * nlabels + label] = the unit of an edge
    // instance `inst` takes from a state where it stands at `label` (the instance's own unit for "Done" and for a label of another process); units 0 .. ninst - 1 are the
    // instances' own ("the remaining labels of the process body"), the units of `-` label sets and of single `+` labels follow.
    // conj_of_unit[u] = the conjuncts unit u belongs to; fair_conj[k]: conjunct k, weak or strong, as text for its instance.
    struct FairConj { bool strong = false; std::string text; };
    std::vector<signed char> unit_of;
    std::vector<unsigned long long> conj_of_unit;
    std::vector<FairConj> fair_conj;
    std::string live_refusal_units;       // "" = the checks by units decide this program's properties; else why not
    std::string translated_labelfair;     // `translated` with the conjuncts above in Spec (the same text for a program without these forms)
    // the cfg's other temporal properties.  live_preds: the distinct state predicates they are made of, compiled after the
    // INVARIANTs and CONSTRAINTs into the same image but never run by the search (a table of their own: the entries are not in the header).
    // live_props: one entry per check — a quantifier instance of a conjunct of a named definition — or per refused name.
    struct LivePred { std::string text; int entry = 0; };
    struct LiveProp { std::string origin, name; int kind = -1, p = -1, q = -1; std::string refusal; };
    std::vector<LivePred> live_preds;
    std::vector<LiveProp> live_props;
    // the cfg's ACTION_CONSTRAINTs and VIEW: code after the live predicates', entries in tables of the program's own
    std::vector<std::string> action_constraints;   // the names, in cfg order
    std::vector<int> acon_entry;                   // one entry per name
    struct ViewComp { int a = 0, n = 0; std::string text; };   // n > 0: the cells a .. a + n - 1 of a variable; n == 0: the code at a (one value)
    std::vector<ViewComp> view;
    std::string view_text;                         // the body of the definition the cfg's VIEW names ("<<c1, ..., ck>>"), or ""
    // the safety parts of the cfg's PROPERTYs.  kind 1 (`[]P`) is one more invariant entry of the image's header, behind
    // the cfg's INVARIANTs (`invariants` stays the cfg's names); kind 0 (`[][A]_v`) and kind 2 (an initial predicate) have their entries in the
    // table behind the image (spec_vm_cfg.h).  index: the invariant index a violation reports (kind 1: its header entry; kind 0: ninv + k;
    // kind 2: behind those).
    struct SafeProp { std::string origin, text; int kind = 0, index = 0, entry = 0; };
    std::vector<SafeProp> safe_props;
    std::vector<std::string> safety_only;          // PROPERTY names without a liveness part whose every conjunct is checked
    std::vector<std::pair<std::string, std::string>> named_conjuncts;   // (PROPERTY, "conjunct `text`: why") beside checked safety parts
    std::vector<int> aprop_entry, initp_entry;     // the entries of kinds 0 and 2, in the order of safe_props
};

// Returns "" or an error message.
std::string compile(const Module &m, const std::string &module_text, const Config &cfg, Program &out);

}  // namespace pcal
