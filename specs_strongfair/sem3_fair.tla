------------------------------ MODULE sem3_fair ------------------------------
(* Written to show: A SEMAPHORE LOCK, 3 processes, declared `fair process`.  A process at `wait` is enabled only while sem = 1: while another holds the lock it is disabled, so it is enabled again and again, never continuously.  Weak fairness lets it starve behind the others' laps; strong fairness does not: on every cycle on which process i stays at `wait` some state has sem = 1, there i is enabled, and i is never taken.  (pc[i] = "wait") ~> (pc[i] = "cs") is VIOLATED.  The twin file differs in the fairness keyword (and the names that carry it) only. *)
EXTENDS Naturals

(* --algorithm sem3_fair
variables sem = 1;

fair process P \in {0, 1, 2}
begin
  ncs:  while TRUE do
  wait:   await sem = 1;
          sem := 0;
  cs:     sem := 1;
        end while;
end process

end algorithm *)

Served == \A i \in {0, 1, 2} : (pc[i] = "wait") ~> (pc[i] = "cs")
=============================================================================
