------------------------------ MODULE refuse_angle ------------------------------
(* <<A>>_v is an action formula no safety check decides. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm refuse_angle
variables x = 0, q = <<>>;
begin
  s: while x < 2 do
       x := x + 1;
     end while;

end algorithm *)

Prop == [][x' >= x]_x /\ <><<x' > x>>_x
=============================================================================
