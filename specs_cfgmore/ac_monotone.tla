------------------------------ MODULE ac_monotone ------------------------------
(* Two processes move x up or down on 0..4, three times each.  ACTION_CONSTRAINT x' >= x refuses every step down: the reachable set and
   the per-level counts change, and at x = 4 every successor is refused. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm ac_monotone
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

Up == x' >= x
=============================================================================
