----------------------------- MODULE many_wrongs -----------------------------
(***************************************************************************)
(* A spec with several wrong invariants at once, written to show what      *)
(* `mc many_wrongs.tla -continue` is for.  N processes bump a counter,     *)
(* take a lock, add the counter to a sum and release the lock — unless the *)
(* sum has grown past 4, where they block for good while holding it.       *)
(*                                                                         *)
(* Without -continue the search stops at depth 3, at the first state in    *)
(* which the lock is held (LockFree), and says nothing about the rest.     *)
(* With it the report lists LockFree, Small and Fresh with the number of   *)
(* states that break each and a shortest behaviour to the first one, the   *)
(* deadlocked states, and Both with 0 states: every state that breaks Both *)
(* breaks Small first, and a state is listed under its first violated      *)
(* invariant only.                                                         *)
(***************************************************************************)
EXTENDS Naturals
CONSTANT N

(* --algorithm many_wrongs
variables x = 0, y = 0, lock = 0;

process P \in 1..N
begin
  a: x := x + 1;
  b: await lock = 0;
     lock := self;
  c: y := y + x;
  d: if y > 4 then
       await FALSE;
     end if;
     lock := 0;
end process

end algorithm *)
\* BEGIN TRANSLATION
VARIABLES x, y, lock, pc

vars == << x, y, lock, pc >>

ProcSet == (1..N)

Init == (* Global variables *)
        /\ x = 0
        /\ y = 0
        /\ lock = 0
        /\ pc = [self \in ProcSet |-> "a"]

a(self) == /\ pc[self] = "a"
           /\ x' = x + 1
           /\ pc' = [pc EXCEPT ![self] = "b"]
           /\ UNCHANGED << y, lock >>

b(self) == /\ pc[self] = "b"
           /\ lock = 0
           /\ lock' = self
           /\ pc' = [pc EXCEPT ![self] = "c"]
           /\ UNCHANGED << x, y >>

c(self) == /\ pc[self] = "c"
           /\ y' = y + x
           /\ pc' = [pc EXCEPT ![self] = "d"]
           /\ UNCHANGED << x, lock >>

d(self) == /\ pc[self] = "d"
           /\ IF y > 4
                 THEN /\ FALSE
                 ELSE /\ TRUE
           /\ lock' = 0
           /\ pc' = [pc EXCEPT ![self] = "Done"]
           /\ UNCHANGED << x, y >>

P(self) == a(self) \/ b(self) \/ c(self) \/ d(self)

Next == (\E self \in 1..N: P(self))
           \/ (* Disjunct to prevent deadlock on termination *)
              ((\A self \in ProcSet: pc[self] = "Done") /\ UNCHANGED vars)

Spec == Init /\ [][Next]_vars

Termination == <>(\A self \in ProcSet: pc[self] = "Done")

\* END TRANSLATION

LockFree == lock = 0
Small == x < N
Fresh == y < 3
Both == y < 3 \/ x < N
=============================================================================
