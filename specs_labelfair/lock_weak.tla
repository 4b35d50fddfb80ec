------------------------------ MODULE lock_weak ------------------------------
(* Written to show: The lock of lock_plus WITHOUT the `+`: under WF_vars(P(self)) alone a process waits for ever while the other laps.  (pc[i] = "wait") ~> (pc[i] = "cs") is VIOLATED. *)
EXTENDS Naturals

(* --algorithm lock_weak
variables sem = 1;

fair process P \in {0, 1}
begin
  ncs:  while TRUE do
  wait:  await sem = 1;
          sem := 0;
  cs:     sem := 1;
        end while;
end process

end algorithm *)

Served == \A i \in {0, 1} : (pc[i] = "wait") ~> (pc[i] = "cs")
=============================================================================
