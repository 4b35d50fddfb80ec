------------------------------ MODULE self_step ------------------------------
(* A fair process whose only step changes no variable, beside an unfair peer that never terminates: the unchanged step is no step of the process, which is therefore never enabled. *)
EXTENDS Naturals

(* --algorithm self_step
variables x = 0;

fair process Idle = 0
begin
  I: while TRUE do
       skip;
     end while;
end process

process Peer = 1
begin
  P: while TRUE do
       x := 1 - x;
     end while;
end process

end algorithm *)
=============================================================================
