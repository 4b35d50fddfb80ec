------------------------------ MODULE ap_done ------------------------------
(* A terminating algorithm: every step of it changes pc, and the terminating disjunct (UNCHANGED vars) is never a violation. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_done
variables x = 0;
begin
  a: x := 1;
  b: x := x + 1;

end algorithm *)

Moves == [][pc' # pc]_vars
=============================================================================
