------------------------------ MODULE ghost_history ------------------------------
(* Two workers read-modify-write a shared cell.  `last` (who wrote last) and `n` (how many writes, saturating at K) are ghosts: nothing
   reads them.  VIEW <<x, pc, t>> leaves both out; it is a congruence, so the viewed search visits the quotient graph. *)
EXTENDS Naturals, Sequences, TLC
CONSTANT K
(* --algorithm ghost_history
variables x = 0, last = 0, n = 0;

process W \in 1..2
variable t = 0;
begin
  rd: t := x;
  wr: x := (t + 1) % 3;
      last := self;
      n := IF n < K THEN n + 1 ELSE n;
  ck: if x # 0 then
        goto rd;
      end if;
end process

end algorithm *)

View == <<x, pc, t>>
=============================================================================
