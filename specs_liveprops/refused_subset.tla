------------------------------ MODULE refused_subset ------------------------------
(* Written to show a REFUSAL: a state predicate outside the expression subset the INVARIANT compiler accepts.  The property is named as NOT checked, with the reason, and the search's own verdict stands. *)
EXTENDS Naturals

(* --algorithm refused_subset
variables x = 0;

fair process Step = 0
begin
  A: x := 1;
end process

end algorithm *)

Odd == <>(SUBSET {x} = {})
=============================================================================
