------------------------------ MODULE starve_leads ------------------------------
(* Written to show: STARVATION UNDER WEAK FAIRNESS as a leads-to.  The algorithm of specs_liveness/starve_wf.tla: a fair waiter awaits turn = 1 while a fair flipper keeps flipping the turn.  The waiter is disabled in every other state of the flipper's cycle, so weak fairness does not oblige it to move, and  (pc[0] = "W") ~> (got = 1)  is VIOLATED. *)
EXTENDS Naturals

(* --algorithm starve_leads
variables turn = 0, got = 0;

fair process Waiter = 0
begin
  W:   await turn = 1;
  Got: got := 1;
end process

fair process Flipper = 1
begin
  F: while got = 0 do
       turn := 1 - turn;
     end while;
end process

end algorithm *)

Served == (pc[0] = "W") ~> (got = 1)
=============================================================================
