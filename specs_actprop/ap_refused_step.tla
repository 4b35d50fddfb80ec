------------------------------ MODULE ap_refused_step ------------------------------
(* ap_monotone once more, with the ACTION_CONSTRAINT x' >= x beside the PROPERTY: the step that breaks Mono is refused by the constraint too, and is still reported. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_refused_step
variables x = 2;

process P \in 1..2
variable c = 0;
begin
  s: while c < 3 do
       either
         await x < 4;
         x := x + 1;
       or
         await x > 0;
         x := x - 1;
       end either;
       c := c + 1;
     end while;
end process

end algorithm *)

Mono == [][x' >= x]_x
Up == x' >= x
=============================================================================
