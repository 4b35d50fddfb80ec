------------------------------ MODULE ac_soup ------------------------------
(* The primed forms of the models with queues and message soups: a whole sequence against a tuple of constants and against itself,
   membership in a primed set of records, a primed set of records against {}, a primed record against itself, UNCHANGED of a record. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm ac_soup
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

Keep == /\ (q' = q \/ q' # <<>>)
        /\ ([type |-> "m", from |-> 1] \in msgs => [type |-> "m", from |-> 1] \in msgs')
        /\ (msgs' = {} => msgs = {})
        /\ (r' = r \/ r'.cnt > r.cnt)
        /\ (msgs' # msgs => UNCHANGED r)
=============================================================================
