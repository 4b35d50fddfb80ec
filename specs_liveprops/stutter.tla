------------------------------ MODULE stutter ------------------------------
(* Written to show: A STUTTERING WITNESS.  x goes from 0 to 1 and the algorithm is Done; x = 2 never holds.  <>(x = 2)  is VIOLATED by the behaviour that takes the one step and then stutters in the Done state for ever (every process is disabled there: the one-state component is fair): the counterexample has an empty cycle. *)
EXTENDS Naturals

(* --algorithm stutter
variables x = 0;

fair process Step = 0
begin
  A: x := 1;
end process

end algorithm *)

Never == <>(x = 2)
=============================================================================
