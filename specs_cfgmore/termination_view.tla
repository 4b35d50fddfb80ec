------------------------------ MODULE termination_view ------------------------------
(* Compiles, but PROPERTY Termination under a VIEW is named as NOT checked: the graph is one of representatives. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm termination_view
variables x = 0, y = 0;

fair process P \in 1..2
begin
  a: x := x + 1;
  b: y := y + x;
end process

end algorithm *)

View == <<x, pc>>
=============================================================================
