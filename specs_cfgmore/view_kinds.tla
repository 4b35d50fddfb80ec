------------------------------ MODULE view_kinds ------------------------------
(* A view whose components are a RECORD variable (all its fields), a SEQUENCE and a SET OF RECORDS; the ghost g (a history sum nothing
   reads) is left out.  The view is a congruence. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm view_kinds
variables r = [cnt |-> 0, flag |-> FALSE], q = <<>>, msgs = {}, g = 0;

process P \in 1..2
begin
  a: r.cnt := r.cnt + 1;
     g := g + self;
  b: q := Append(q, self);
  c: msgs := msgs \cup {[type |-> "m", from |-> self]};
     g := g + 1;
end process

end algorithm *)

View == <<r, q, msgs, pc>>
=============================================================================
