------------------------------ MODULE ap_soup ------------------------------
(* A set of records (a message soup) under [][Cardinality(msgs') >= Cardinality(msgs)]_msgs: it only grows.  Under NoLoss2 (at most one message is ever added) the second send breaks the property. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_soup
variables msgs = {};

process P \in 1..2
variable c = 0;
begin
  s: while c < 2 do
       either
         msgs := msgs \cup {[type |-> "m", from |-> self]};
       or
         msgs := msgs \cup {[type |-> "n", from |-> self]};
       end either;
       c := c + 1;
     end while;
end process

end algorithm *)

KCard == [][Cardinality(msgs') >= Cardinality(msgs)]_msgs
AtMostOne == [][Cardinality(msgs') <= 1]_msgs
=============================================================================
