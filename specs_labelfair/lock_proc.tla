------------------------------ MODULE lock_proc ------------------------------
(* Written to show: THE LOCK OF lock_plus WITH acquire AS A PROCEDURE whose label `wait:+` is strongly fair: beside WF_vars of the process's own labels and WF_vars of acquire's labels the process gets SF_vars(wait(self)) — here the label's copy wait_p1.  (pc[i] = "wait_p1") ~> (pc[i] = "cs") HOLDS; without the `+` it would be violated as in lock_weak. *)
EXTENDS Naturals

(* --algorithm lock_proc
variables sem = 1;

procedure acquire()
begin
  wait:+ await sem = 1;
         sem := 0;
         return;
end procedure

fair process P \in {0, 1}
begin
  ncs:  while TRUE do
          call acquire();
  cs:     sem := 1;
        end while;
end process

end algorithm *)

Served == \A i \in {0, 1} : (pc[i] = "wait_p1") ~> (pc[i] = "cs")
=============================================================================
