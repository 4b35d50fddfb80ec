------------------------------ MODULE ac_two ------------------------------
(* Two action constraints, a CONSTRAINT and an INVARIANT.  The step x := x + 3 from the initial state is refused by Slow, and its successor
   (x = 3) still violates Inv: the violation is reported, at trace length 2, although that successor is never stored. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm ac_two
variables x = 0, y = 0;

process P \in 1..2
begin
  a: either
       x := x + 1;
     or
       x := x + 3;
     or
       y := y + 1;
     or
       await y > 0;
       y := y - 1;
     end either;
  b: if x + y < 5 then
       goto a;
     end if;
end process

end algorithm *)

Slow == x' <= x + 1
YUp == y' >= y /\ (UNCHANGED <<x, y>> \/ x' + y' > x + y)
Small == y <= 2
Inv == x # 3
=============================================================================
