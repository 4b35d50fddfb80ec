------------------------------ MODULE leftover ------------------------------
(* Written to show: A ONE-STATE FINAL COMPONENT LEFT OVER AFTER THE REFINEMENT, as a <>[]P case and a stuttering witness.  An unfair process flips x between 0 and 1; a strongly fair one is enabled at x = 1 only and ends it there.  The component {0, 1} is blocked (Kick is enabled in it, never taken), the state x = 1 leaves, and x = 0 alone is left: no fair process is enabled there, so the behaviour may stutter in it for ever.  <>[](x # 0) and <>(x = 2) are VIOLATED, the counterexample ends in `Stuttering` at x = 0. *)
EXTENDS Naturals

(* --algorithm leftover
variables x = 0;

fair+ process Kick = 0
begin
  K: await x = 1;
     x := 2;
end process

process Flip = 1
begin
  M: while x < 2 do
       x := 1 - x;
     end while;
end process

end algorithm *)

Settles == <>[](x # 0)
Kicked == <>(x = 2)
=============================================================================
