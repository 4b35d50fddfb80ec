----------------------------- MODULE dead_label -----------------------------
(***************************************************************************)
(* A spec with a label no process ever reaches, written to show what       *)
(* `mc dead_label.tla -coverage` is for.  Two workers take turns through a *)
(* critical section and count their visits; the branch to Panic is guarded *)
(* by `hits > 2`, which cannot hold with two workers that enter once each. *)
(* The model checker reports "No error has been found" either way: only    *)
(* the coverage statistics show that Panic never fired (its row is 0:0),   *)
(* so whatever Panic was meant to exercise has not been checked.           *)
(***************************************************************************)
EXTENDS Naturals

(* --algorithm dead_label
variables turn = 0, hits = 0;

process Worker \in 1..2
begin
  Enter:
    await turn = 0;
    turn := self;
  Work:
    hits := hits + 1;
  Check:
    if hits > 2 then
      goto Panic;
    else
      goto Leave;
    end if;
  Panic:
    hits := 0;
  Leave:
    turn := 0;
end process

end algorithm *)
\* BEGIN TRANSLATION
VARIABLES turn, hits, pc

vars == << turn, hits, pc >>

ProcSet == (1..2)

Init == (* Global variables *)
        /\ turn = 0
        /\ hits = 0
        /\ pc = [self \in ProcSet |-> "Enter"]

Enter(self) == /\ pc[self] = "Enter"
               /\ turn = 0
               /\ turn' = self
               /\ pc' = [pc EXCEPT ![self] = "Work"]
               /\ UNCHANGED hits

Work(self) == /\ pc[self] = "Work"
              /\ hits' = hits + 1
              /\ pc' = [pc EXCEPT ![self] = "Check"]
              /\ UNCHANGED turn

Check(self) == /\ pc[self] = "Check"
               /\ IF hits > 2
                     THEN /\ pc' = [pc EXCEPT ![self] = "Panic"]
                     ELSE /\ pc' = [pc EXCEPT ![self] = "Leave"]
               /\ UNCHANGED << turn, hits >>

Panic(self) == /\ pc[self] = "Panic"
               /\ hits' = 0
               /\ pc' = [pc EXCEPT ![self] = "Leave"]
               /\ UNCHANGED turn

Leave(self) == /\ pc[self] = "Leave"
               /\ turn' = 0
               /\ pc' = [pc EXCEPT ![self] = "Done"]
               /\ UNCHANGED hits

Worker(self) == Enter(self) \/ Work(self) \/ Check(self) \/ Panic(self) \/ Leave(self)

Next == (\E self \in 1..2: Worker(self))
           \/ (* Disjunct to prevent deadlock on termination *)
              ((\A self \in ProcSet: pc[self] = "Done") /\ UNCHANGED vars)

Spec == Init /\ [][Next]_vars

Termination == <>(\A self \in ProcSet: pc[self] = "Done")

\* END TRANSLATION

Bounded == hits <= 2
OneAtATime == \A w \in 1..2 : pc[w] \in {"Work", "Check", "Panic", "Leave"} => turn = w
=============================================================================
