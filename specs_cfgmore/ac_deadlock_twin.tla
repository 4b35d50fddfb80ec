------------------------------ MODULE ac_deadlock_twin ------------------------------
(* ac_deadlock's twin: the same refusal as a state CONSTRAINT. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm ac_deadlock_twin
variables x = 0;

process P = 1
begin
  a: x := 1;
  b: x := 5;
  c: x := 6;
end process

end algorithm *)

Small == x <= 4
=============================================================================
