------------------------------ MODULE ap_monotone ------------------------------
(* ac_monotone's algorithm under PROPERTY Mono: the first step down breaks [][x' >= x]_x; the behaviour has two states. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_monotone
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
