------------------------------ MODULE spin_minus ------------------------------
(* Written to show: A FAIR PROCESS whose spinning label is `spin:-`, beside a plain fair Setter.  The Spinner's conjunct is WF_vars((pc[0] \notin {"spin"}) /\ Spinner): no fairness for the action at `spin`.  The Setter ends the loop condition, but nothing obliges the Spinner to take its last step out of `spin`: Termination is VIOLATED, through that label only (the behaviour stutters with flag = 1 and the Spinner still at `spin`).  The twin spin_fair differs in the `-` only. *)
EXTENDS Naturals

(* --algorithm spin_minus
variables flag = 0, turns = 0;

fair process Spinner = 0
begin
  spin:- while flag = 0 do
          turns := 1 - turns;
        end while;
end process

fair process Setter = 1
begin
  set: flag := 1;
end process

end algorithm *)

=============================================================================
