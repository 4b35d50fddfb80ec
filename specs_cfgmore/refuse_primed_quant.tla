------------------------------ MODULE refuse_primed_quant ------------------------------
(* Refused, by a message that names the form: a quantifier over a primed set of records. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm refuse_primed_quant
variables q = <<>>, msgs = {}, r = [cnt |-> 0, flag |-> FALSE];

process P \in 1..2
variable c = 0;
begin
  s: while c < 2 do
       either
         q := Append(q, self);
       or
         await Len(q) > 0;
         q := Tail(q);
       or
         msgs := msgs \cup {[type |-> "m", from |-> self]};
       or
         msgs := msgs \ {[type |-> "m", from |-> self]};
       or
         r := [cnt |-> r.cnt + 1, flag |-> TRUE];
       or
         r := [cnt |-> 0, flag |-> r.flag];
       end either;
       c := c + 1;
     end while;
end process

end algorithm *)

Bad == \A m \in msgs' : m.from > 0
=============================================================================
