------------------------------ MODULE ap_seen ------------------------------
(* x runs 0, 1, 2, 0, ...: the only step that breaks [][x' > x]_x is 2 -> 0, and it ends in the initial state, stored long before. Only a check of every GENERATED successor finds it; the behaviour has four states. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_seen
variables x = 0;
begin
  s: while TRUE do
       x := (x + 1) % 3;
     end while;

end algorithm *)

Up == [][x' > x]_x
=============================================================================
