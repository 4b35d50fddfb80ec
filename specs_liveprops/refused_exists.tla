------------------------------ MODULE refused_exists ------------------------------
(* Written to show a REFUSAL: an existential quantifier over a temporal formula.  The property is named as NOT checked, with the reason, and the search's own verdict stands. *)
EXTENDS Naturals

(* --algorithm refused_exists
variables x = 0;

fair process Step = 0
begin
  A: x := 1;
end process

end algorithm *)

Some == \E i \in {0, 1} : <>(x = i)
=============================================================================
