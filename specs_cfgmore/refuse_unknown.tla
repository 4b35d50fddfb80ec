------------------------------ MODULE refuse_unknown ------------------------------
(* Refused: the cfg names an action constraint the module does not define. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm refuse_unknown
variables x = 0, y = 0;

process P \in 1..2
begin
  a: x := x + 1;
  b: y := y + x;
end process

end algorithm *)

Other == x' >= x
=============================================================================
