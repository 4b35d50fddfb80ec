------------------------------ MODULE ap_spec ------------------------------
(* The usual refinement shape HInit /\ [][HNext]_hv /\ WF_hv(HNext): the initial predicate and the step formula are checked, the fairness conjunct is named.  HSpecStrict lacks the disjunct for label t's step; HSpecOne asks for another initial state. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_spec
variables x = 0, y = 0;

process P = 1
begin
  s: while x < 2 do
       x := x + 1;
     end while;
  t: y := x;
end process

end algorithm *)

hv == <<x, y>>
HInit == x = 0 /\ y = 0
HNext == \/ (x' = x + 1 /\ y' = y)
         \/ (y' = x /\ x' = x)
HStrict == x' = x + 1 /\ y' = y
HSpec == HInit /\ [][HNext]_hv /\ WF_hv(HNext)
HSpecStrict == HInit /\ [][HStrict]_hv /\ WF_hv(HStrict)
HSpecOne == (x = 1) /\ [][HNext]_hv
=============================================================================
