"""<>Q, []<>Q, <>[]P and P ~> Q without a GPU: the front end (which definitions become checks, under which names, over which
predicates; what is refused and why; that a cfg without such a property compiles to what it compiled to before), the reference the GPU
tests rely on (tests/liveprops.py: checked against what the models under specs_liveprops/ were written to show, and against a
brute-force reading of the definition), and liveness.h itself — through tests/_livepropshim, a g++ build of the rule with sequential
components and a sequential reach pass, which must give the reference's answers on every model while five mutants of it do not."""
import ctypes as C
import hashlib
import json

import pytest

import helpers
import liveprops

ROOT = helpers.ROOT


@pytest.fixture(scope="module")
def amd():
    import tla_rust_amd
    return tla_rust_amd


@pytest.fixture(scope="module")
def graphs():
    """(Program, PropGraph) per model, built once and shared: nothing changes them"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = liveprops.load(name)
        return made[name]
    yield get
    for prog, _ in made.values():
        prog.close()


# ------------------------------------------------------------------------------------------------ the front end
HEAD = "---- MODULE m ----\nEXTENDS Naturals\nCONSTANTS K, Names\n(* --algorithm m\nvariables x = 0, y = 0;\nfair process P \\in 0..1\nbegin\n  A: x := 1;\n  B: y := 1;\nend process\nend algorithm *)\n"
CFG = "SPECIFICATION Spec\nCONSTANTS K = 2 Names = {\"a\", \"b\"}\nPROPERTY Prop\n"


DEFS = "Seen == x = 1\nHeld(i) == x = i\n"   # (names the accepted bodies apply)


def props_of(amd, body, cfg=CFG, more=DEFS):
    p = amd.Program(HEAD + more + "Prop == " + body + "\n====\n", cfg)
    try:
        return [dict(lp) for lp in p.live_properties], list(p.live_predicates)
    finally:
        p.close()


ACCEPTED = [   # body, [(name, kind, predicate texts P / Q)]
    ("<>(x = 1)", [("Prop", 2, None, "( x = 1 )")]),
    ("<>Seen", [("Prop", 2, None, "Seen")]),
    ("<>~(x = 1)", [("Prop", 2, None, "~ ( x = 1 )")]),
    ("[]<>Held(0)", [("Prop", 1, None, "Held ( 0 )")]),
    ("<>[]Held(1)", [("Prop", 3, "Held ( 1 )", None)]),
    ("(<>(x = 1))", [("Prop", 2, None, "( x = 1 )")]),
    ("<>((x = 1) \\/ (y = 5))", [("Prop", 2, None, "( ( x = 1 ) \\/ ( y = 5 ) )")]),
    ("(x = 0) \\/ (y = 0) ~> (y = 1) \\/ (x = 7)", [("Prop", 0, "( x = 0 ) \\/ ( y = 0 )", "( y = 1 ) \\/ ( x = 7 )")]),
    ("(IF x = 0 THEN x = 1 ELSE y = 0) ~> (y = 1)", [("Prop", 0, "( IF x = 0 THEN x = 1 ELSE y = 0 )", "( y = 1 )")]),
    ("x = 0 /\\ (\\A j \\in {0, 1} : y # j + 5) ~> (y = 1)", [("Prop", 0, "x = 0 /\\ ( \\A j \\in { 0 , 1 } : y # j + 5 )", "( y = 1 )")]),
    ("(x = 0) ~> \\A j \\in {0, 1} : y # j + 5", [("Prop", 0, "( x = 0 )", "\\A j \\in { 0 , 1 } : y # j + 5")]),
    ("<>(x = 1) /\\ \\A i \\in 0..1 : <>(y = i)", [("Prop.1", 2, None, "( x = 1 )"), ("Prop.2[i = 0]", 2, None, "( y = i ) | i = 0"), ("Prop.2[i = 1]", 2, None, "( y = i ) | i = 1")]),
    ("((x = 0) => (x = 1)) ~> (y = 1)", [("Prop", 0, "( ( x = 0 ) => ( x = 1 ) )", "( y = 1 )")]),
    ("[]<>(x = 1)", [("Prop", 1, None, "( x = 1 )")]),
    ("<>[](x = 1)", [("Prop", 3, "( x = 1 )", None)]),
    ("(x = 0) ~> (y = 1)", [("Prop", 0, "( x = 0 )", "( y = 1 )")]),
    ("((x = 0) ~> (y = 1))", [("Prop", 0, "( x = 0 )", "( y = 1 )")]),
    ("x = 0 /\\ y = 0 ~> y = 1", [("Prop", 0, "x = 0 /\\ y = 0", "y = 1")]),
    ("TRUE ~> (y = 1)", [("Prop", 0, "TRUE", "( y = 1 )")]),
    ("\\A i \\in 0..1 : (pc[i] = \"A\") ~> (pc[i] = \"Done\")",
     [("Prop[i = 0]", 0, "( pc [ i ] = \"A\" ) | i = 0", "( pc [ i ] = \"Done\" ) | i = 0"),
      ("Prop[i = 1]", 0, "( pc [ i ] = \"A\" ) | i = 1", "( pc [ i ] = \"Done\" ) | i = 1")]),
    ("\\A i \\in 1..K : <>(x = i)", [("Prop[i = 1]", 2, None, "( x = i ) | i = 1"), ("Prop[i = 2]", 2, None, "( x = i ) | i = 2")]),
    ("\\A i \\in ProcSet : \\A j \\in {3} : <>(x = i + j)", [("Prop[i = 0, j = 3]", 2, None, "( x = i + j ) | i = 0 | j = 3"), ("Prop[i = 1, j = 3]", 2, None, "( x = i + j ) | i = 1 | j = 3")]),
    ("\\A n \\in Names : <>(x = 1)", [("Prop[n = \"a\"]", 2, None, "( x = 1 )"), ("Prop[n = \"b\"]", 2, None, "( x = 1 )")]),
    ("<>(x = 1) /\\ []<>(y = 1)", [("Prop.1", 2, None, "( x = 1 )"), ("Prop.2", 1, None, "( y = 1 )")]),
    ("\n  /\\ <>(x = 1)\n  /\\ (x = 1) ~> (y = 1)", [("Prop.1", 2, None, "( x = 1 )"), ("Prop.2", 0, "( x = 1 )", "( y = 1 )")]),
    ("\\A i \\in 0..1 : <>(x = i) /\\ <>[](y = 1)", [("Prop.1[i = 0]", 2, None, "( x = i ) | i = 0"), ("Prop.1[i = 1]", 2, None, "( x = i ) | i = 1"),
                                                   ("Prop.2[i = 0]", 3, "( y = 1 )", None), ("Prop.2[i = 1]", 3, "( y = 1 )", None)]),
]


@pytest.mark.parametrize("body,want", ACCEPTED, ids=[b for b, _ in ACCEPTED])
def test_accepted_forms_become_checks(amd, body, want):
    props, preds = props_of(amd, body)
    assert not any(lp["refused"] for lp in props) and all(lp["origin"] == "Prop" for lp in props)
    got = [(lp["name"], lp["kind"], preds[lp["p"]] if lp["p"] >= 0 else None, preds[lp["q"]] if lp["q"] >= 0 else None) for lp in props]
    assert got == want
    assert len(set(preds)) == len(preds)   # deduplicated


def test_predicates_are_shared_between_checks(amd):
    props, preds = props_of(amd, "\\A i \\in 0..1 : (pc[i] = \"A\") ~> (y = 1)")
    assert preds == ["( pc [ i ] = \"A\" ) | i = 0", "( y = 1 )", "( pc [ i ] = \"A\" ) | i = 1"]   # Q does not mention i: one predicate, one mask
    assert [(lp["p"], lp["q"]) for lp in props] == [(0, 1), (2, 1)]
    cfg = CFG.replace("PROPERTY Prop", "PROPERTIES Prop Other Prop Termination")
    props, preds = props_of(amd, "<>(y = 1)", cfg, more="Other == []<>(y = 1)\n")
    assert [(lp["origin"], lp["kind"], lp["q"]) for lp in props] == [("Prop", 2, 0), ("Other", 1, 0)] and preds == ["( y = 1 )"]   # (a name twice: once; Termination: not here)


REFUSED = [   # body, the reason's key word
    # a temporal prefix operator binds tighter than every infix operator: these are NOT <>(A op B), and none of the four shapes
    ("<>x = 1", "parenthesised"),
    ("<>(x = 1) \\/ (y = 5)", "parenthesised"),
    ("<>(x = 1) => (y = 5)", "parenthesised"),
    ("[]<>(x = 1) \\/ (y = 1)", "parenthesised"),
    ("[]<>(x = 1) \\lor (y = 1)", "parenthesised"),
    ("<>[](x = 1) <=> (y = 1)", "parenthesised"),
    ("<>[](x = 1) \\equiv (y = 1)", "parenthesised"),
    ("<>(x = 1) + 1", "parenthesised"),
    ("<>(x = 1) /\\ <>(y = 1) \\/ <>(y = 2)", "nested"),
    # ... and => / <=> bind looser than ~>: A => (B ~> C)
    ("(x = 0) => (x = 1) ~> (y = 1)", "looser"),
    ("(x = 0) ~> (x = 1) => (y = 1)", "looser"),
    ("(x = 0) <=> (x = 1) ~> (y = 1)", "looser"),
    ("(x = 0) \\equiv (x = 1) ~> (y = 1)", "looser"),
    # ... and IF / LET / CASE / CHOOSE / a quantifier inside a larger expression reach as far right as they can
    ("IF x = 0 THEN x = 1 ELSE y = 0 ~> (y = 1)", "as far right"),
    ("LET z == 1 IN x = z ~> (y = 1)", "as far right"),
    ("CASE x = 0 -> y = 0 [] OTHER -> y = 1 ~> (y = 1)", "as far right"),
    ("x = 0 /\\ \\A j \\in {0, 1} : y = j ~> (y = 1)", "as far right"),
    ("x = 0 /\\ \\E j \\in {0, 1} : y = j ~> (y = 1)", "as far right"),
    ("x = (CHOOSE j \\in {0, 1} : TRUE) /\\ y = CHOOSE j \\in {0, 1} : j = 1 ~> (y = 1)", "as far right"),
    ("<>(x = 1) /\\ \\A i \\in {} : <>(y = 5) /\\ <>(y = 7)", "as far right"),
    ("<>(x = 1) /\\ \\A i \\in 0..1 : <>(y = i) /\\ <>(y = 7)", "as far right"),
    ("(<>(x = 1)) \\/ (<>(y = 1))", "not one of"),
    ("\\A i \\in {} : <>(x = i)", "no check"),
    ("<>[]<>(x = 1)", "nested"),
    ("[]<>(<>(x = 1))", "nested"),
    ("(x = 0) ~> (y = 0) ~> (x = 1)", "nested"),
    ("(x = 0) ~> <>(y = 1)", "nested"),
    ("[](x = 1)", "safety"),
    ("[][x' = x]_x", "safety"),
    ("\\E i \\in 0..1 : <>(x = i)", "\\E"),
    ("<>(x' = 1)", "primed"),
    ("<>(x = 1) /\\ WF_vars(Next)", "WF_"),
    ("<>(SF_vars(Next))", "SF_"),
    ("<>(SUBSET {x} = {})", "subset"),
    ("<>(x = CHOOSE n \\in Nat : n > 3)", "subset"),
    ("\\A i \\in 0..16 : <>(x = i)", "16 checks"),
    ("\\A i \\in 0..5 : \\A j \\in 0..5 : (x = i) ~> (y = j)", "16 checks"),
    ("\\A i \\in 0..x : <>(y = i)", "constant set"),
    ("<>(x = 1) /\\ (y = 1)", "not one of"),
]


@pytest.mark.parametrize("body,word", REFUSED, ids=[b for b, _ in REFUSED])
def test_refused_forms_name_their_reason(amd, body, word):
    props, preds = props_of(amd, body)
    assert len(props) == 1 and props[0]["refused"] and props[0]["kind"] == -1 and (props[0]["origin"], props[0]["name"]) == ("Prop", "Prop")
    assert word in props[0]["reason"], props[0]["reason"]
    assert preds == []   # as if the name had never been compiled


def test_more_than_32_predicates_and_names_that_are_no_temporal_definitions(amd):
    many = " /\\ ".join(f"<>(x = {k})" for k in range(33))
    props, preds = props_of(amd, many)
    assert len(props) == 1 and props[0]["refused"] and ("16 checks" in props[0]["reason"] or "32 distinct" in props[0]["reason"])
    cfg = CFG.replace("PROPERTY Prop", "PROPERTIES A1 A2 A3 Nowhere Inv")
    more = "".join(f"A{j} == \\A i \\in 0..5 : (x = i + {j}) ~> (y = i + {j})\n" for j in (1, 2, 3)) + "Inv == x < 2\n"
    props, preds = props_of(amd, "<>(x = 1)", cfg, more=more)
    by = {}
    for lp in props:
        by.setdefault(lp["origin"], []).append(lp)
    assert [len(by[k]) for k in ("A1", "A2", "A3")] == [6, 6, 1] and "16 checks" in by["A3"][0]["reason"] and len(preds) == 24
    assert by["Nowhere"][0]["refused"] and "not a definition" in by["Nowhere"][0]["reason"]
    assert by["Inv"][0]["refused"] and "state-level" in by["Inv"][0]["reason"]
    long = "P" * 63
    cfg = CFG.replace("PROPERTY Prop", f"PROPERTIES {long} {long}x")   # 63 characters are a name; 64 are refused, and do not borrow the other's checks
    props, preds = props_of(amd, "<>(x = 1)", cfg, more=f"{long} == <>(x = 1)\n{long}x == <>(y = 1)\n")
    assert [(lp["origin"] == long, lp["refused"]) for lp in props] == [(True, False), (True, True)] and "63 characters" in props[1]["reason"] and len(preds) == 1


@pytest.mark.parametrize("stem", list(liveprops.REFUSED))
def test_the_refusal_models(amd, stem):
    name, word = liveprops.REFUSED[stem]
    p = liveprops.compiled(stem)
    try:
        assert [(lp["origin"], lp["refused"]) for lp in p.live_properties] == [(name, True)] and word in p.live_properties[0]["reason"]
        assert p.live_predicates == [] and p.live_refusal is None
    finally:
        p.close()


# ---- a cfg that names no such property compiles to what it compiled to before
def image_of(prog):
    import livepropshim
    L = livepropshim.lib()
    L.livepropshim_image.restype = C.c_long
    L.livepropshim_image.argtypes = [C.POINTER(helpers.McSpecDesc), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_int64)]
    d = helpers.spec_desc("pcal", prog.params)
    fields = (C.c_int64 * 22)()
    n = L.livepropshim_image(C.byref(d), None, 0, fields)
    assert n > 0
    image = (C.c_int32 * n)()
    assert L.livepropshim_image(C.byref(d), image, n, fields) == n
    return bytes(image), list(fields)


def header_of(amd, prog):
    L = amd.binding.lib()
    L.mc_program_codegen.restype = C.c_long
    L.mc_program_codegen.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    n = L.mc_program_codegen(prog._h, None, 0)
    if n < 0:
        return None   # (a program the translator to generated code does not cover: the same before and after)
    buf = C.create_string_buffer(n + 1)
    L.mc_program_codegen(prog._h, buf, n + 1)
    return buf.value.decode()


def old_cfgs():
    out = []
    for d in (ROOT / "specs" / "pluscal", ROOT / "specs_liveness"):
        for cfg in sorted(d.glob("*.cfg")):
            tla = cfg.with_suffix(".tla")
            if not tla.exists():   # (a second cfg of a module: ring_1000.cfg -> ring.tla)
                tla = next((t for t in sorted(d.glob("*.tla")) if cfg.stem.startswith(t.stem)), None)
            if tla is not None:
                out.append((tla, cfg))
    return out


GOLDEN = ROOT / "tests" / "golden" / "liveprops_images.json"


def digest(image, fields, header):
    return hashlib.sha256(image + json.dumps(fields).encode() + (header or "").encode()).hexdigest()


def test_a_cfg_without_such_a_property_compiles_to_what_it_did(amd):
    """image, VmParams and generated header of every cfg under specs/pluscal and specs_liveness: none names such a property, so no
    predicate is compiled; the digests are the ones recorded from the front end as it was before it knew these properties
    (tests/golden/liveprops_images.json), which covers the checkpoint's identity too — it hashes the image and these fields; and
    naming a property the front end refuses changes none of the three"""
    golden = json.loads(GOLDEN.read_text())
    pairs = old_cfgs()
    assert len(pairs) >= 30 and {str(c.relative_to(ROOT)) for _, c in pairs} == set(golden)
    for tla, cfg in pairs:
        text, ctext = tla.read_text(), cfg.read_text()
        try:
            p = amd.Program(text, ctext)
        except amd.McError:
            assert golden[str(cfg.relative_to(ROOT))] is None, cfg   # (a cfg the compiler refuses, then as now)
            continue
        try:
            assert p.live_predicates == [] and all(lp["refused"] for lp in p.live_properties), cfg
            image, fields = image_of(p)
            header = header_of(amd, p)
            assert digest(image, fields, header) == golden[str(cfg.relative_to(ROOT))], cfg
            q = amd.Program(text, ctext + "\nPROPERTY NoSuchDefinitionAnywhere\n")
            try:
                assert image_of(q) == (image, fields) and header_of(amd, q) == header, cfg
                assert [lp["refused"] for lp in q.live_properties if lp["origin"] == "NoSuchDefinitionAnywhere"] == [True]
            finally:
                q.close()
        finally:
            p.close()


def test_a_name_refused_after_its_predicates_were_compiled_leaves_nothing_behind(amd):
    """17 checks, more than 32 predicates, a predicate the compiler refuses after others of the same name went through — each with a
    string literal nothing else mentions: image, VmParams and generated header are those of the cfg without the property, and a
    property compiled after the refused one gets what it gets without it"""
    vars_ = HEAD.replace("variables x = 0, y = 0;", "variables x = 0, y = 0, s = \"a\";")
    bodies = {"Many": "\\A i \\in 0..16 : <>((x = i) /\\ (s = \"fresh\"))",
              "Wide": " /\\ ".join(f"<>((x = {k}) /\\ (s = \"w{k}\"))" for k in range(33)),
              "Late": "<>(s = \"late\") /\\ <>(x = CHOOSE n \\in Nat : n > 3)"}
    text = vars_ + "".join(f"{n} == {b}\n" for n, b in bodies.items()) + "Good == <>(s = \"a\")\n====\n"
    base = "SPECIFICATION Spec\nCONSTANTS K = 2 Names = {\"a\", \"b\"}\n"
    p0, pg = amd.Program(text, base), amd.Program(text, base + "PROPERTY Good\n")
    try:
        want0, wantg = (image_of(p0), header_of(amd, p0)), (image_of(pg), header_of(amd, pg), list(pg.live_predicates))
        for name in bodies:
            p = amd.Program(text, base + f"PROPERTY {name}\n")
            q = amd.Program(text, base + f"PROPERTIES {name} Good\n")
            try:
                assert [lp["refused"] for lp in p.live_properties] == [True] and p.live_predicates == [], name
                assert (image_of(p), header_of(amd, p)) == want0, name
                assert (image_of(q), header_of(amd, q), list(q.live_predicates)) == wantg, name
            finally:
                p.close()
                q.close()
    finally:
        p0.close()
        pg.close()


def test_an_evaluation_error_inside_a_predicate_is_an_error_of_the_check(amd, tmp_path):
    import livepropshim
    p = liveprops.compiled("pred_error")
    try:
        with pytest.raises(RuntimeError, match="-7"):   # MC_ESTATE, no verdict
            livepropshim.check(p, p.fair_mask, p.live_properties[0], tmp_path)
    finally:
        p.close()


def test_predicates_are_appended_and_leave_the_rest_alone(amd):
    """with a property, the image is the old image plus the predicates' code (only the header's code length differs), and the generated
    header gains run_inv cases and nothing else"""
    text = (liveprops.DIR / "starve_leads.tla").read_text()
    p0, p1 = amd.Program(text, "SPECIFICATION Spec\n"), amd.Program(text, "SPECIFICATION Spec\nPROPERTY Served\n")
    try:
        (i0, f0), (i1, f1) = image_of(p0), image_of(p1)
        a, b = memoryview(i0).cast("i"), memoryview(i1).cast("i")
        differ = [k for k in range(len(a)) if a[k] != b[k]]
        assert len(b) > len(a) and len(differ) == 1 and a[differ[0]] == len(a) and b[differ[0]] == len(b)   # VMH_CODE_LEN
        assert [k for k in range(22) if f0[k] != f1[k]] == [11]   # code_len
        h0, h1 = header_of(amd, p0), header_of(amd, p1)
        assert h0 != h1 and "case 1: return inv1(v, result);" in h1 and "inv0" not in h0
        assert p0.translated() == p1.translated() == amd.pcal_translate(text)   # translate() does not know the cfg
    finally:
        p0.close()
        p1.close()


# ------------------------------------------------------------------------------------------------ the reference
def checks_of(prog):
    return [lp for lp in prog.live_properties if not lp["refused"]]


@pytest.mark.parametrize("name", list(liveprops.MODELS))
def test_the_reference_gives_the_verdict_the_model_was_written_for(graphs, name):
    prog, g = graphs(name)
    got = {lp["name"]: liveprops.decide_model(g, lp, prog.fair_mask).violated for lp in checks_of(prog)}
    assert got == liveprops.MODELS[name].expect
    if name == "leave_enabled":   # the fair process is enabled in both states of the cycle, by the edge that leaves the mask
        v = liveprops.decide_model(g, checks_of(prog)[0], prog.fair_mask)
        assert v.mask_states == 2 and not v.violating and all(1 in g.en[i] for i in range(len(g.texts)) if not g.bits[i] >> 1 & 1)
    if name == "mask_split":      # one component of G, three one-state components of G[M] and the Q state
        v = liveprops.decide_model(g, checks_of(prog)[0], prog.fair_mask)
        assert len(set(g.comp)) == 1 and len(set(v.comp)) == 3 and v.mask_states == 2
    if name == "stutter":
        v = liveprops.decide_model(g, checks_of(prog)[0], prog.fair_mask)
        assert len(v.path) == 2 and len(v.root) == 1 and not g.en[v.path[-1]]
    if name == "ring_cut":
        v = liveprops.decide_model(g, checks_of(prog)[0], prog.fair_mask)
        assert len(v.path) == 33 and v.bad_starts == 31 + 2 and v.mask_states == 65 - 2 + 2


def test_the_reference_equals_the_definition_on_every_small_model(graphs):
    done = []
    for name in liveprops.SMALL:
        prog, g = graphs(name)
        for lp in checks_of(prog):
            brute = liveprops.brute_force(g, lp, prog.fair_mask)
            assert brute is not None, f"{name} {lp['name']}: M holds more than {liveprops.BRUTE_CAP} states"
            assert brute == liveprops.decide_model(g, lp, prog.fair_mask).violated, (name, lp["name"])
            done.append((name, lp["name"]))
    assert {n for n, _ in done} == set(liveprops.SMALL) and len(done) == sum(len(liveprops.MODELS[n].expect) for n in liveprops.SMALL)
    # and under another fairness assumption than the model's own: nobody fair, everybody fair
    for name in liveprops.SMALL:
        prog, g = graphs(name)
        for fair in (0, (1 << g.nproc) - 1):
            for lp in checks_of(prog):
                assert liveprops.brute_force(g, lp, fair) == liveprops.decide_model(g, lp, fair).violated, (name, lp["name"], fair)


# ------------------------------------------------------------------------------------------------ liveness.h on the host
def check_model(name, tmp, graphs, L=None):
    import livepropshim
    prog, g = graphs(name)
    for lp in checks_of(prog):
        got = livepropshim.check(prog, prog.fair_mask, lp, tmp, L=L)
        assert got["states"] == len(g.texts) and got["preds"] == len(prog.live_predicates)
        assert dict(zip(got["texts"], got["bits"])) == dict(zip(g.texts, g.bits)), f"{name}: the predicate bits differ from the reference's"
        rank = {t: i for i, t in enumerate(got["texts"])}
        want = liveprops.decide_model(g, lp, prog.fair_mask, rank=[rank[t] for t in g.texts])
        texts = lambda c: frozenset(g.texts[v] for v in c)   # noqa: E731
        assert got["violating"] == {texts(c) for c in want.violating}, f"{name} {lp['name']}: the violating components differ from the reference's"
        assert got["witness"] == (g.texts[want.witness] if want.violated else None), f"{name} {lp['name']}: the witness differs from the reference's"
        assert (got["mask_states"], got["bad_starts"]) == (want.mask_states, want.bad_starts), f"{name} {lp['name']}: the counts differ from the reference's"
        if want.violated:
            assert [got["dist"][g.texts[v]] for v in want.path] == list(range(len(want.path) - 1, -1, -1))


@pytest.mark.parametrize("name", list(liveprops.MODELS))
def test_the_rule_on_the_host_equals_the_reference(name, tmp_path, graphs):
    check_model(name, tmp_path, graphs)


# name: (its text in liveness.h, the replacement, the model that must catch it)
MUTANTS = {
    "en-from-the-masked-graph": ("en_ |= 1ull << p;", "if (in_m(dst[k])) en_ |= 1ull << p;", "leave_enabled"),
    "components-of-the-whole-graph": ("return !live_in_mask(c, bits);", "return false;", "mask_split"),
    "reach-ignores-the-mask": ("MC_HD bool live_passable(const LiveCheck &c, uint32_t bits) {\n    return live_in_mask(c, bits);",
                               "MC_HD bool live_passable(const LiveCheck &c, uint32_t bits) {\n    return true;", "reach_mask"),
    "all-states-in-T": ("c.done = c.done || done;", "c.done = c.first ? done : (c.done && done);", "stable"),
    "eventually-from-all-states": ("if (c.kind == LIVE_EVENTUALLY) return initial;", "if (c.kind == LIVE_EVENTUALLY) return true;", "lost"),
}


def test_mutants_of_the_rule_are_caught(tmp_path, graphs):
    import livepropshim
    import testlib
    helpers.build_shim()

    def build(name):
        return livepropshim.build(csrc=testlib.mutant_tree(tmp_path, name, ("liveness.h", *MUTANTS[name][:2])), out=tmp_path / name / "_build")
    for name, so in testlib.build_mutants(MUTANTS, build).items():
        run = tmp_path / name / "run"
        run.mkdir()
        with pytest.raises(AssertionError) as e:
            check_model(MUTANTS[name][2], run, graphs, L=livepropshim.load(so))
            pytest.fail(f"mutant {name} survives", pytrace=False)
        assert "from the reference's" in str(e.value), (name, str(e.value)[:300])
