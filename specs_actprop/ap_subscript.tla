------------------------------ MODULE ap_subscript ------------------------------
(* A steps x, B steps y.  [][x' = x + 1]_x holds: B's steps stutter on x.  Under the subscript <<x, y>> they do not, and B's first step breaks it. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_subscript
variables x = 0, y = 0;

process A = 1
begin
  a: while x < 3 do
       x := x + 1;
     end while;
end process

process B = 2
variable n = 0;
begin
  b: while n < 2 do
       y := 1 - y;
       n := n + 1;
     end while;
end process

end algorithm *)

IncX == [][x' = x + 1]_x
IncXY == [][x' = x + 1]_<<x, y>>
=============================================================================
