------------------------------ MODULE lock_plus ------------------------------
(* Written to show: A SEMAPHORE LOCK whose `wait` label ALONE is strongly fair (`wait:+` in a `fair process`).  A process at `wait` is enabled only while sem = 1, again and again but never continuously: WF_vars(P(self)) lets it starve, the conjunct SF_vars(wait(self)) that the `+` adds does not.  (pc[i] = "wait") ~> (pc[i] = "cs") HOLDS.  The twin lock_weak differs in the `+` only. *)
EXTENDS Naturals

(* --algorithm lock_plus
variables sem = 1;

fair process P \in {0, 1}
begin
  ncs:  while TRUE do
  wait:+  await sem = 1;
          sem := 0;
  cs:     sem := 1;
        end while;
end process

end algorithm *)

Served == \A i \in {0, 1} : (pc[i] = "wait") ~> (pc[i] = "cs")
=============================================================================
