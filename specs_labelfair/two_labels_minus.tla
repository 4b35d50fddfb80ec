------------------------------ MODULE two_labels_minus ------------------------------
(* Written to show: A `-` label that is ONE of two labels of a fair process: the Setter may rest at `idle:-` for ever (its conjunct WF_vars((pc[1] \notin {"idle"}) /\ Setter) is disabled there) while the fair Spinner spins: Termination is VIOLATED by a cycle, not by stuttering.  With the `-` counted into the conjunct the Setter would have to move and Termination would hold. *)
EXTENDS Naturals

(* --algorithm two_labels_minus
variables flag = 0, turns = 0;

fair process Spinner = 0
begin
  spin: while flag = 0 do
          turns := 1 - turns;
        end while;
end process

fair process Setter = 1
begin
  idle:- skip;
  set:  flag := 1;
end process

end algorithm *)

=============================================================================
