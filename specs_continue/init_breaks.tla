----------------------------- MODULE init_breaks -----------------------------
(***************************************************************************)
(* The initial state itself breaks an invariant: a violator without a      *)
(* parent, at depth 1.  `mc init_breaks.tla -continue` lists Positive with *)
(* the states in which the counter is still 0 and Low with the ones that   *)
(* have counted past 2.                                                    *)
(***************************************************************************)
EXTENDS Naturals

(* --algorithm init_breaks
variables n = 0;

process Q \in 1..2
begin
  up: n := n + 1;
  again: n := n + 1;
end process

end algorithm *)
\* BEGIN TRANSLATION
VARIABLES n, pc

vars == << n, pc >>

ProcSet == (1..2)

Init == (* Global variables *)
        /\ n = 0
        /\ pc = [self \in ProcSet |-> "up"]

up(self) == /\ pc[self] = "up"
            /\ n' = n + 1
            /\ pc' = [pc EXCEPT ![self] = "again"]

again(self) == /\ pc[self] = "again"
               /\ n' = n + 1
               /\ pc' = [pc EXCEPT ![self] = "Done"]

Q(self) == up(self) \/ again(self)

Next == (\E self \in 1..2: Q(self))
           \/ (* Disjunct to prevent deadlock on termination *)
              ((\A self \in ProcSet: pc[self] = "Done") /\ UNCHANGED vars)

Spec == Init /\ [][Next]_vars

Termination == <>(\A self \in ProcSet: pc[self] = "Done")

\* END TRANSLATION

Positive == n > 0
Low == n < 3
=============================================================================
