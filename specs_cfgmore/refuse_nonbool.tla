------------------------------ MODULE refuse_nonbool ------------------------------
(* Refused: an action constraint that is no Boolean-valued formula. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm refuse_nonbool
variables x = 0, y = 0;

process P \in 1..2
begin
  a: x := x + 1;
  b: y := y + x;
end process

end algorithm *)

Num == x' + 1
=============================================================================
