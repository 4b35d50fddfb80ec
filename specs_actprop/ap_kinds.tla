------------------------------ MODULE ap_kinds ------------------------------
(* One property per primed kind: pc'[i], a per-process local, a record field, Len of a sequence, a set of naturals (ap_soup has the set of records).  KBad (the queue keeps its length) is broken by the first Append. *)
EXTENDS Naturals, Sequences, FiniteSets, TLC

(* --algorithm ap_kinds
variables r = [cnt |-> 0, flag |-> FALSE], q = <<>>, S = {};

process P \in 1..2
variable c = 0;
begin
  s: while c < 2 do
       either
         r.cnt := r.cnt + 1;
       or
         q := Append(q, self);
       or
         S := S \cup {self};
       end either;
       c := c + 1;
     end while;
end process

end algorithm *)

KPc == [][\A i \in 1..2 : pc'[i] = pc[i] \/ pc[i] = "s"]_pc
KLocal == [][\A i \in 1..2 : c'[i] >= c[i]]_c
KField == [][r'.cnt >= r.cnt]_r
KLen == [][Len(q') >= Len(q)]_q
KSet == [][S \subseteq S']_S
KBad == [][Len(q') = Len(q)]_q
=============================================================================
