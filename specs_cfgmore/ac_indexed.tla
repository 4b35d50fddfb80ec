------------------------------ MODULE ac_indexed ------------------------------
(* A primed FUNCTION under a quantifier: label b may add 2 to the process's own counter, which the action constraint refuses. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm ac_indexed
variables tries = [i \in 1..2 |-> 0];

process P \in 1..2
begin
  a: tries[self] := tries[self] + 1;
  b: either
       tries[self] := tries[self] + 2;
     or
       skip;
     end either;
  c: if tries[self] < 3 then
       goto a;
     end if;
end process

end algorithm *)

Gentle == \A i \in ProcSet : tries'[i] <= tries[i] + 1
=============================================================================
