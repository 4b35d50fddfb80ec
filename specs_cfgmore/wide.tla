------------------------------ MODULE wide ------------------------------
(* Four processes, four alternatives each (17 slots per state): small frontiers take the slot-sliced launches, the widest levels more than
   one workgroup.  The ghost g (a history sum nothing reads) is left out by the VIEW, and the action constraint refuses the step by two of the first two processes. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm wide
variables x = [i \in 1..4 |-> 0], g = 0;

process P \in 1..4
variable c = 0;
begin
  s: while c < 1 do
       either
         x[self] := (x[self] + 1) % 3;
         g := g + self;
       or
         x[self] := (x[self] + 2) % 3;
         g := g + 2 * self;
       or
         x[self] := 0;
       or
         g := g + 1;
       end either;
       c := c + 1;
     end while;
end process

end algorithm *)

View == <<x, pc, c>>
Gentle == \A i \in 1..2 : x'[i] <= x[i] + 1
=============================================================================
