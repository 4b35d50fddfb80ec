----------------------------- MODULE outside_only -----------------------------
(***************************************************************************)
(* The only states that break the invariant lie outside the CONSTRAINT:    *)
(* they are generated and checked, never stored.  `mc outside_only.tla     *)
(* -continue` lists Under with 0 distinct states and the number of such    *)
(* successors, and its behaviour ends in the successor itself.             *)
(***************************************************************************)
EXTENDS Naturals

(* --algorithm outside_only
variables n = 0;

process R \in 1..2
begin
  one: n := n + 1;
  two: n := n + 2;
end process

end algorithm *)
\* BEGIN TRANSLATION
VARIABLES n, pc

vars == << n, pc >>

ProcSet == (1..2)

Init == (* Global variables *)
        /\ n = 0
        /\ pc = [self \in ProcSet |-> "one"]

one(self) == /\ pc[self] = "one"
             /\ n' = n + 1
             /\ pc' = [pc EXCEPT ![self] = "two"]

two(self) == /\ pc[self] = "two"
             /\ n' = n + 2
             /\ pc' = [pc EXCEPT ![self] = "Done"]

R(self) == one(self) \/ two(self)

Next == (\E self \in 1..2: R(self))
           \/ (* Disjunct to prevent deadlock on termination *)
              ((\A self \in ProcSet: pc[self] = "Done") /\ UNCHANGED vars)

Spec == Init /\ [][Next]_vars

Termination == <>(\A self \in ProcSet: pc[self] = "Done")

\* END TRANSLATION

Under == n < 5
Bound == n < 5
=============================================================================
