------------------------------ MODULE self_step_exit ------------------------------
(* A fair process that may either stay where it is (a step that changes nothing) or go on: weak fairness obliges it to go on, since the unchanged step does not count as taken.  Termination holds. *)
EXTENDS Naturals

(* --algorithm self_step_exit
variables x = 0;

fair process Dither = 0
begin
  L: either goto L;
     or x := 1;
     end either;
end process

end algorithm *)
=============================================================================
