------------------------------ MODULE refuse_subscript ------------------------------
(* The subscript is no variable tuple. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm refuse_subscript
variables x = 0, q = <<>>;
begin
  s: while x < 2 do
       x := x + 1;
     end while;

end algorithm *)

Prop == [][x' >= x]_<<x + 1>>
=============================================================================
