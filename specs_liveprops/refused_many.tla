------------------------------ MODULE refused_many ------------------------------
(* Written to show a REFUSAL: more checks than a cfg may ask for: 17 quantifier instances.  The property is named as NOT checked, with the reason, and the search's own verdict stands. *)
EXTENDS Naturals

(* --algorithm refused_many
variables x = 0;

fair process Step = 0
begin
  A: x := 1;
end process

end algorithm *)

Many == \A i \in 0..16 : <>(x = i)
=============================================================================
