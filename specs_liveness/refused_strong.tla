------------------------------ MODULE refused_strong ------------------------------
(* fair+ asks for strong fairness: Termination is not checked. *)
EXTENDS Naturals

(* --algorithm refused_strong
variables x = 0;

fair+ process P = 0
begin
  A: x := 1;
end process

end algorithm *)
=============================================================================
