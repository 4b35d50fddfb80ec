------------------------------ MODULE leave_enabled ------------------------------
(* Written to show: LEAVING COUNTS AS ENABLED.  While q = 0 an unfair process flips x: a cycle of two ~Q states.  The fair process's only step, q := 1, leads out of the cycle into a Q state.  In the cycle it is never disabled (en is taken in the full graph: the edge that leaves the mask still enables it) and never taken, so the cycle is unfair and  (q = 0) ~> (q = 1)  HOLDS. *)
EXTENDS Naturals

(* --algorithm leave_enabled
variables x = 0, q = 0;

process Spin = 0
begin
  S: while q = 0 do
       x := 1 - x;
     end while;
end process

fair process Leave = 1
begin
  L: q := 1;
end process

end algorithm *)

Reaches == (q = 0) ~> (q = 1)
=============================================================================
