------------------------------ MODULE refuse_next ------------------------------
(* A names the translation's own Next. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm refuse_next
variables x = 0, q = <<>>;
begin
  s: while x < 2 do
       x := x + 1;
     end while;

end algorithm *)

Prop == [][Next]_vars
=============================================================================
