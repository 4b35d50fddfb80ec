------------------------------ MODULE refused_nested ------------------------------
(* Written to show a REFUSAL: a temporal operator under another one.  The property is named as NOT checked, with the reason, and the search's own verdict stands. *)
EXTENDS Naturals

(* --algorithm refused_nested
variables x = 0;

fair process Step = 0
begin
  A: x := 1;
end process

end algorithm *)

Deep == <>[]<>(x = 1)
=============================================================================
