------------------------------ MODULE ac_deadlock ------------------------------
(* After label a the only successor (x := 5) is refused by the action constraint: a state ALL of whose successors are refused.  The verdict
   is what the twin ac_deadlock_twin gets with a CONSTRAINT of the same effect. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm ac_deadlock
variables x = 0;

process P = 1
begin
  a: x := 1;
  b: x := 5;
  c: x := 6;
end process

end algorithm *)

Step == x' - x <= 2
=============================================================================
