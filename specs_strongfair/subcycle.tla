------------------------------ MODULE subcycle ------------------------------
(* Written to show: VIOLATED EVEN UNDER `fair+`, FOUND ONLY IN ROUND 2.  A fair walker moves x over 0 -> 1 -> (0 or 2) and 2 -> 0; a strongly fair process can end it all at x = 2 only.  The three states are one component in which Exit is enabled (at x = 2) and never taken: no fair suffix passes all three.  Without the state x = 2 the component 0 <-> 1 is left, Exit is disabled in both of its states, the walker is taken: a fair suffix after all, which the second round of the refinement finds.  Termination and <>(x = 9) are VIOLATED, and the cycle printed never passes x = 2. *)
EXTENDS Naturals

(* --algorithm subcycle
variables x = 0;

fair+ process Exit = 0
begin
  E: await x = 2;
     x := 9;
end process

fair process Walk = 1
begin
  L: while x < 9 do
       if x = 1 then
         either x := 0 or x := 2 end either;
       elsif x = 2 then
         x := 0;
       else
         x := 1;
       end if;
     end while;
end process

end algorithm *)

Leaves == <>(x = 9)
Gone == (x = 1) ~> (x = 9)
=============================================================================
