------------------------------ MODULE ap_two ------------------------------
(* Out of the initial state, A's step breaks the INVARIANT and KeepX at once (the invariant is what is reported), B's step breaks KeepY: two properties and one invariant violated in one level. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_two
variables x = 0, y = 0;

process A = 1
begin
  a: x := 2;
end process

process B = 2
begin
  b: y := 1;
end process

end algorithm *)

Inv == x < 2
KeepX == [][x' <= 1]_x
KeepY == [][y' = y]_y
=============================================================================
