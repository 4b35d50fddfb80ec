------------------------------ MODULE peterson_loop ------------------------------
(* Written to show: STARVATION FREEDOM OF A PETERSON LOOP, two instances from one definition.  Each process announces itself and yields the turn in one step (a1), waits until the other is not interested or the turn is its own (wait), and leaves (cs) to start over.  Only process i ever gives the turn away from i, and it does so before it waits.  While i waits with the turn the other's, the other is enabled in every state (at wait because the turn is its own, at cs and a1 always), so weak fairness makes it go round to a1, which hands the turn to i; from then on i is enabled in every state until it moves, and weak fairness makes it move.  So  \A i \in {0, 1} : (pc[i] = "wait") ~> (pc[i] = "cs")  HOLDS for both instances. *)
EXTENDS Naturals

(* --algorithm peterson_loop
variables flag = [i \in {0, 1} |-> FALSE], turn = 0;

fair process Proc \in {0, 1}
begin
  a1:   flag[self] := TRUE || turn := 1 - self;
  wait: await ~flag[1 - self] \/ turn = self;
  cs:   flag[self] := FALSE;
        goto a1;
end process

end algorithm *)

Starvation == \A i \in {0, 1} : (pc[i] = "wait") ~> (pc[i] = "cs")
=============================================================================
