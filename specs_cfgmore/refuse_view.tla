------------------------------ MODULE refuse_view ------------------------------
(* Refused: a view component that is neither a variable nor a scalar expression of the subset. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm refuse_view
variables x = 0, y = 0;

process P \in 1..2
begin
  a: x := x + 1;
  b: y := y + x;
end process

end algorithm *)

View == <<x, {y, 1}>>
=============================================================================
