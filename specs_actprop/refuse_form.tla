------------------------------ MODULE refuse_form ------------------------------
(* A primed form outside the subset: a primed sequence against an expression. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm refuse_form
variables x = 0, q = <<>>;
begin
  s: while x < 2 do
       x := x + 1;
     end while;

end algorithm *)

Prop == [][q' = Tail(q)]_q
=============================================================================
