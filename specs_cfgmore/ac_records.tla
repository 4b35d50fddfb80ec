------------------------------ MODULE ac_records ------------------------------
(* Primes on a record FIELD and on Len of a sequence: the counter field never goes down, the queue never shrinks. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm ac_records
variables r = [cnt |-> 0, flag |-> FALSE], q = <<>>;

process P \in 1..2
variable c = 0;
begin
  s: while c < 2 do
       either
         r.cnt := r.cnt + 1;
       or
         r := [cnt |-> 0, flag |-> TRUE];
       or
         q := Append(q, self);
       or
         await Len(q) > 0;
         q := Tail(q);
       end either;
       c := c + 1;
     end while;
end process

end algorithm *)

Grow == r'.cnt >= r.cnt /\ Len(q') >= Len(q)
=============================================================================
