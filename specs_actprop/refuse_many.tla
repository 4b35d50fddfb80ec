------------------------------ MODULE refuse_many ------------------------------
(* More than 8 action properties in one cfg. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm refuse_many
variables x = 0, q = <<>>;
begin
  s: while x < 2 do
       x := x + 1;
     end while;

end algorithm *)

P0 == [][x' >= x - 0]_x
P1 == [][x' >= x - 1]_x
P2 == [][x' >= x - 2]_x
P3 == [][x' >= x - 3]_x
P4 == [][x' >= x - 4]_x
P5 == [][x' >= x - 5]_x
P6 == [][x' >= x - 6]_x
P7 == [][x' >= x - 7]_x
P8 == [][x' >= x - 8]_x
=============================================================================
